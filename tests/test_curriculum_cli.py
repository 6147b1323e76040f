"""The geodesic curriculum on the vnav.train command line: --geo-curriculum LEVEL [--cur-window N
--cur-up P --cur-down Q --cur-step K --cur-min L --cur-mode 1|2] reach the trainer's arguments."""
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
    assert train.main(["cached-thor", "--geo-curriculum", "3"]) == 0
    assert seen[0]["geo_curriculum"] == dict(level=3)
    del seen[:]
    assert train.main(["cached-thor", "--geo-curriculum", "1", "--cur-window", "64", "--cur-up", "0.9", "--cur-down",
                       "0.25", "--cur-step", "2", "--cur-min", "2", "--cur-mode", "2", "--cuda-graph"]) == 0
    assert seen[0]["geo_curriculum"] == dict(level=1, window=64, up=0.9, down=0.25, step=2, level_min=2, mode=2)
    assert seen[0]["cuda_graph"] is True
    del seen[:]
    for bad in (["cached-thor", "--cur-window", "64"], ["cached-thor", "--geo-curriculum", "1", "--cur-mode", "3"],
                ["cached-thor", "--cur-mode", "1"]):
        with pytest.raises(SystemExit):
            train.main(bad)
    assert not seen


def test_experiment_passes_it_on():
    """The experiment attribute is the trainer's argument; every key is one of
    VectorEnv.set_geodesic_curriculum's parameters."""
    import inspect

    from vnav import train
    from vnav.envs import VectorEnv
    exp = train.make_trainer("cached-thor", geo_curriculum=dict(level=2, window=8))
    assert exp.geo_curriculum == dict(level=2, window=8)
    assert train.make_trainer("cached-thor").geo_curriculum is None
    names = set(inspect.signature(VectorEnv.set_geodesic_curriculum).parameters) - {"self"}
    assert names == {"level", "mode", "window", "up", "down", "step", "level_min"}
    assert "geo_curriculum=self.geo_curriculum" in inspect.getsource(train.Experiment.create_trainer)
