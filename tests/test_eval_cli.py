"""The fixed-episode evaluation on the vnav.train command line: --test --eval-episodes N
[--eval-buckets ...] [--greedy] [--eval-set FILE] [--save-eval-set FILE]."""
import numpy as np
import pytest


def test_flags_reach_test_episodes(monkeypatch):
    from vnav import train
    seen = []

    class Exp:
        def test(self, episodes=None):
            seen.append(("test", episodes))

        def test_episodes(self, **kw):
            seen.append(("test_episodes", kw))

        def run(self, resume=False):
            seen.append(("run", resume))

    monkeypatch.setattr(train, "make_trainer", lambda name, **kw: Exp())
    monkeypatch.setattr(train.vdist, "init_distributed", lambda: None)
    assert train.main(["cached-thor", "--test", "--episodes", "7"]) == 0
    assert seen.pop() == ("test", 7)  # without the new flags --test is what it was
    assert train.main(["cached-thor", "--test", "--eval-episodes", "4", "--eval-buckets", "1-2,3-", "--greedy",
                       "--save-eval-set", "s.npz"]) == 0
    assert seen.pop() == ("test_episodes", dict(per_bucket=4, buckets=((1, 2), (3, None)), greedy=True, eval_set=None,
                                                save_eval_set="s.npz", max_episode_steps=None))
    assert train.main(["cached-thor", "--test", "--eval-set", "s.npz", "--eval-max-steps", "30"]) == 0
    assert seen.pop() == ("test_episodes", dict(per_bucket=None, buckets=None, greedy=False, eval_set="s.npz",
                                                save_eval_set=None, max_episode_steps=30))
    for bad in (["cached-thor", "--test", "--greedy"], ["cached-thor", "--eval-episodes", "4"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


@pytest.mark.gpu
def test_saved_set_gives_identical_tables(tmp_path, monkeypatch):
    """--test --eval-episodes 4 --save-eval-set, then --eval-set on the same checkpoint, through
    main(): the same episodes, the same tables. Plain --test keeps its keys."""
    from vnav import train
    logs = []
    kw = dict(env_kwargs=dict(grid=(6, 6), frame=(84, 84), goal=(3, 3, 0), num_envs=8), save_dir=str(tmp_path),
              max_time_steps=8 * 20 * 2, saving_period=0, episode_log_interval=0, logger=logs.append)
    train.make_trainer("thor-cached-auxiliary", **kw).run()
    path = str(tmp_path / "episodes.npz")
    made = []
    real = train.make_trainer

    def small(name, env_kwargs=None, save_dir=None, seed=0, **over):
        # the command line's experiment on the small scene the checkpoint was trained on
        assert not env_kwargs and not over
        made.append(real(name, **dict(kw, save_dir=save_dir, seed=seed)))
        return made[-1]

    monkeypatch.setattr(train, "make_trainer", small)
    base = ["thor-cached-auxiliary", "--test", "--save-dir", str(tmp_path), "--eval-max-steps", "15"]

    def tables(*args):
        logs.clear()
        assert train.main(base + list(args)) == 0
        return [l for l in logs if l.startswith("---")]

    t1 = tables("--eval-episodes", "4", "--save-eval-set", path)
    saved = np.load(path)
    assert set(saved.files) == {"scene", "start", "goal", "distance", "buckets"}
    assert saved["buckets"].tolist() == [[1, 3], [4, 8], [9, -1]]
    filled = len(np.unique(np.searchsorted([4, 9], saved["distance"], side="right")))
    assert len(saved["scene"]) == 4 * filled and filled >= 2 and (saved["distance"] >= 1).all()
    t2 = tables("--eval-set", path)
    assert t1 == t2 and len(t1) == 4  # one table per bucket and one over all episodes
    for col in ("distance", "success_rate", "spl", "start_distance", "episodes", "reward", "episode_length"):
        assert all("| " + col in t for t in t1), col
    assert "| 1-3" in t1[0] and "| 9-" in t1[2] and "| all" in t1[-1]
    assert ("| %-8d" % len(saved["scene"])) in [l for l in t1[-1].split("\n") if l.startswith("| episodes")][0]
    t3 = tables("--eval-set", path, "--greedy")
    assert len(t3) == 4
    env = made[-1].trainer.env
    assert env.max_episode_steps == 900 and env.episode_log is None and env.error_flags() == 0
    # plain --test: the keys it had
    monkeypatch.setattr(train, "make_trainer", real)
    res = train.make_trainer("thor-cached-auxiliary", **kw).test(episodes=3)
    assert set(res) == {"episodes", "reward", "episode_length", "success_rate", "spl", "start_distance"}
