"""PPO minibatches on the vnav.train command line: --ppo-minibatches M reaches the trainer's
ppo_minibatches, is refused without --ppo-clip and below 1, and the experiment passes it on with
the trainer's own default (1 = full-batch epochs)."""
import pytest


def test_flag_reaches_the_trainer(monkeypatch):
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
    assert train.main(["cached-thor", "--ppo-clip", "0.2"]) == 0
    assert seen == [dict(base, ppo_clip=0.2), "run"]  # without the flag nothing is passed
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.2", "--ppo-minibatches", "4"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.2, ppo_minibatches=4)
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.1", "--ppo-epochs", "3", "--ppo-minibatches", "1",
                       "--optimizer", "adam"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.1, ppo_epochs=3, ppo_minibatches=1, optimizer="adam")
    del seen[:]
    for bad in (["cached-thor", "--ppo-minibatches", "2"], ["cached-thor", "--ppo-clip", "0.2", "--ppo-minibatches", "0"],
                ["cached-thor", "--ppo-clip", "0.2", "--ppo-minibatches", "-3"],
                ["cached-thor", "--optimizer", "adam", "--ppo-minibatches", "2"],
                ["cached-thor", "--ppo-clip", "0.2", "--ppo-minibatches", "two"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_it_on():
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    exp = train.make_trainer("cached-thor", ppo_clip=0.2, ppo_minibatches=8)
    assert exp.ppo_minibatches == 8
    off = train.make_trainer("cached-thor")
    assert off.ppo_minibatches == 1
    params = inspect.signature(A2CTrainer.__init__).parameters
    assert params["ppo_minibatches"].default == 1
    assert "ppo_minibatches=self.ppo_minibatches" in inspect.getsource(train.Experiment.create_trainer)
    # the argument is the last one: positional callers of the trainer are not disturbed
    assert list(params)[-1] == "ppo_minibatches"
