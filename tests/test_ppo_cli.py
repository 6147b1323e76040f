"""PPO and Adam on the vnav.train command line: --ppo-clip C, --ppo-epochs K, --ppo-value-clip CV,
--no-adv-norm and --optimizer reach the trainer's arguments; the dependent flags without
--ppo-clip and values out of range are refused; the metric vector gains its last segment."""
import pytest


def test_flags_reach_the_trainer(monkeypatch):
    from vnav import train
    seen = []

    class Exp:
        def run(self, resume=False):
            seen.append("run")

    def make(name, **kw):
        seen.append(kw)
        return Exp()

    monkeypatch.setattr(train, "make_trainer", make)
    monkeypatch.setattr(train.vdist, "init_distributed", lambda: None)
    base = dict(env_kwargs={}, save_dir=None, seed=0)
    assert train.main(["cached-thor"]) == 0
    assert seen == [base, "run"]  # without the flags nothing is passed
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.2"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.2)
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.1", "--ppo-epochs", "3", "--ppo-value-clip", "0.5",
                       "--no-adv-norm", "--optimizer", "adam", "--gae-lambda", "0.95"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.1, ppo_epochs=3, ppo_value_clip=0.5, ppo_normalize_advantage=False,
                           optimizer="adam", gae_lambda=0.95)
    del seen[:]
    assert train.main(["cached-thor", "--optimizer", "adam"]) == 0  # Adam needs no PPO
    assert seen[0] == dict(base, optimizer="adam")
    del seen[:]
    for bad in (["cached-thor", "--ppo-epochs", "2"], ["cached-thor", "--ppo-value-clip", "0.2"],
                ["cached-thor", "--no-adv-norm"], ["cached-thor", "--ppo-clip", "0"],
                ["cached-thor", "--ppo-clip", "-0.2"], ["cached-thor", "--ppo-clip", "0.2", "--ppo-epochs", "0"],
                ["cached-thor", "--ppo-clip", "0.2", "--ppo-value-clip", "-1"],
                ["cached-thor", "--optimizer", "sgd"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_them_on():
    """The experiment attributes are the trainer's arguments, off by default."""
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    names = ("ppo_clip", "ppo_epochs", "ppo_value_clip", "ppo_normalize_advantage", "optimizer")
    exp = train.make_trainer("cached-thor", ppo_clip=0.2, ppo_epochs=2, ppo_value_clip=0.3,
                             ppo_normalize_advantage=False, optimizer="adam")
    assert tuple(getattr(exp, k) for k in names) == (0.2, 2, 0.3, False, "adam")
    off = train.make_trainer("cached-thor")
    assert tuple(getattr(off, k) for k in names) == (None, 4, 0.0, True, "rmsprop")
    params = inspect.signature(A2CTrainer.__init__).parameters
    src = inspect.getsource(train.Experiment.create_trainer)
    for name in names:
        assert "%s=self.%s" % (name, name) in src
        assert params[name].default == getattr(off, name)
    assert params["adam_betas"].default == (0.9, 0.999) and params["adam_epsilon"].default == 1e-5


def test_metric_segment_rides_last():
    from vnav.metrics import metric_layout
    assert metric_layout(ppo=True) == {"base": (0, 9), "ppo": (9, 4)}
    assert metric_layout(novelty=True, ppo=True) == {"base": (0, 9), "novelty": (9, 3), "ppo": (12, 4)}
    full = metric_layout(True, True, True, True, True, True, True, ppo=True)
    assert list(full)[-1] == "ppo" and full["ppo"] == (31, 4) and full["novelty"] == (28, 3)
    # the positional order the trainer uses is unchanged: ppo is the last keyword
    assert metric_layout(True, True, True, True, True, True, True) == {k: v for k, v in full.items() if k != "ppo"}
    assert metric_layout(True, True, True, True, True, True, True, True) == full
