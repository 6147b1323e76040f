"""The visit counts and the novelty bonus on the vnav.train command line: --novelty-weight W,
--first-visit-weight W, --novelty-anneal STEPS and --visit-counts reach the trainer's arguments;
negative weights and a negative anneal are refused."""
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
    assert train.main(["cached-thor", "--novelty-weight", "0.1"]) == 0
    assert seen[0] == dict(base, novelty_weight=0.1)
    del seen[:]
    assert train.main(["cached-thor", "--first-visit-weight", "0.05", "--visit-counts"]) == 0
    assert seen[0] == dict(base, first_visit_weight=0.05, visit_counts=True)
    del seen[:]
    assert train.main(["cached-thor", "--novelty-weight", "0.1", "--first-visit-weight", "0.2", "--novelty-anneal",
                       "100000", "--shaping-weight", "0.5", "--cuda-graph"]) == 0
    assert seen[0] == dict(base, novelty_weight=0.1, first_visit_weight=0.2, novelty_anneal_steps=100000,
                           shaping_weight=0.5, cuda_graph=True)
    del seen[:]
    for bad in (["cached-thor", "--novelty-weight", "-0.1"], ["cached-thor", "--first-visit-weight", "-1"],
                ["cached-thor", "--novelty-weight", "0.1", "--novelty-anneal", "-5"],
                ["cached-thor", "--novelty-anneal", "1000"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_them_on():
    """The experiment attributes are the trainer's arguments, off by default."""
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    names = ("novelty_weight", "first_visit_weight", "novelty_anneal_steps")
    exp = train.make_trainer("cached-thor", novelty_weight=0.1, first_visit_weight=0.2, novelty_anneal_steps=1000,
                             visit_counts=True)
    assert tuple(getattr(exp, k) for k in names) == (0.1, 0.2, 1000) and exp.visit_counts is True
    off = train.make_trainer("cached-thor")
    assert tuple(getattr(off, k) for k in names) == (0.0, 0.0, 0) and off.visit_counts is False
    params = inspect.signature(A2CTrainer.__init__).parameters
    src = inspect.getsource(train.Experiment.create_trainer)
    for name in names:
        assert "%s=self.%s" % (name, name) in src
        assert params[name].default == getattr(off, name)
    assert "set_visit_counts(True)" in inspect.getsource(train.Experiment._setup)


def test_metric_segment_rides_last():
    from vnav.metrics import metric_layout
    assert metric_layout(novelty=True) == {"base": (0, 9), "novelty": (9, 3)}
    full = metric_layout(True, True, True, True, True, True, True)
    assert list(full)[-1] == "novelty" and full["novelty"] == (28, 3)
    assert metric_layout(True, True, True, True, True, True) == {k: v for k, v in full.items() if k != "novelty"}
