"""Reward shaping and GAE on the vnav.train command line: --shaping-weight W [--shaping-gamma G
--shaping-anneal STEPS] and --gae-lambda L reach the trainer's arguments."""
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
    assert train.main(["cached-thor"]) == 0
    assert seen == [dict(env_kwargs={}, save_dir=None, seed=0), "run"]  # without the flags nothing is passed
    del seen[:]
    assert train.main(["cached-thor", "--shaping-weight", "0.25"]) == 0
    assert seen[0] == dict(env_kwargs={}, save_dir=None, seed=0, shaping_weight=0.25)
    del seen[:]
    assert train.main(["cached-thor", "--gae-lambda", "0.95"]) == 0
    assert seen[0] == dict(env_kwargs={}, save_dir=None, seed=0, gae_lambda=0.95)
    del seen[:]
    assert train.main(["cached-thor", "--shaping-weight", "0.5", "--shaping-gamma", "0.99", "--shaping-anneal",
                       "100000", "--gae-lambda", "0.9", "--cuda-graph"]) == 0
    assert seen[0] == dict(env_kwargs={}, save_dir=None, seed=0, shaping_weight=0.5, shaping_gamma=0.99,
                           shaping_anneal_steps=100000, gae_lambda=0.9, cuda_graph=True)
    del seen[:]
    for bad in (["cached-thor", "--shaping-gamma", "0.99"], ["cached-thor", "--shaping-anneal", "1000"],
                ["cached-thor", "--gae-lambda", "1.5"], ["cached-thor", "--gae-lambda", "0.9", "--shaping-anneal", "5"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_them_on():
    """The experiment attributes are the trainer's arguments, off by default."""
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    exp = train.make_trainer("cached-thor", shaping_weight=0.5, shaping_gamma=0.99, shaping_anneal_steps=1000,
                             gae_lambda=0.95)
    assert (exp.shaping_weight, exp.shaping_gamma, exp.shaping_anneal_steps, exp.gae_lambda) == (0.5, 0.99, 1000, 0.95)
    off = train.make_trainer("cached-thor")
    assert (off.shaping_weight, off.shaping_gamma, off.shaping_anneal_steps, off.gae_lambda) == (None, 1.0, 0, 1.0)
    params = inspect.signature(A2CTrainer.__init__).parameters
    src = inspect.getsource(train.Experiment.create_trainer)
    for name in ("shaping_weight", "shaping_gamma", "shaping_anneal_steps", "gae_lambda"):
        assert "%s=self.%s" % (name, name) in src
        assert params[name].default == getattr(off, name)
