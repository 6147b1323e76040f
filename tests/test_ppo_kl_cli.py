"""The target-KL stop on the vnav.train command line: --ppo-target-kl KL and --ppo-kl-host-stop
reach the trainer's ppo_target_kl / ppo_kl_host_stop, each refusal says what is missing, the
experiment passes both on with the trainer's own defaults (off), and the metric segment rides last."""
import pytest


def _patched(monkeypatch):
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
    return train, seen


def test_flags_reach_the_trainer(monkeypatch):
    train, seen = _patched(monkeypatch)
    base = dict(env_kwargs={}, save_dir=None, seed=0)
    assert train.main(["cached-thor", "--ppo-clip", "0.2"]) == 0
    assert seen == [dict(base, ppo_clip=0.2), "run"]  # without the flags nothing is passed
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.2", "--ppo-target-kl", "0.01"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.2, ppo_target_kl=0.01)
    del seen[:]
    assert train.main(["cached-thor", "--ppo-clip", "0.2", "--ppo-minibatches", "4", "--ppo-target-kl", "0.03",
                       "--ppo-kl-host-stop", "--no-cuda-graph"]) == 0
    assert seen[0] == dict(base, ppo_clip=0.2, ppo_minibatches=4, ppo_target_kl=0.03, ppo_kl_host_stop=True,
                           cuda_graph=False)


@pytest.mark.parametrize("argv, message", [
    (["--ppo-target-kl", "0.01"], "--ppo-target-kl needs --ppo-clip"),
    (["--optimizer", "adam", "--ppo-target-kl", "0.01"], "--ppo-target-kl needs --ppo-clip"),
    (["--ppo-clip", "0.2", "--ppo-target-kl", "0"], "--ppo-target-kl must be > 0"),
    (["--ppo-clip", "0.2", "--ppo-target-kl", "-0.01"], "--ppo-target-kl must be > 0"),
    (["--ppo-clip", "0.2", "--ppo-target-kl", "nan"], "--ppo-target-kl must be > 0"),
    (["--ppo-clip", "0.2", "--ppo-kl-host-stop"], "--ppo-kl-host-stop needs --ppo-target-kl"),
    (["--ppo-clip", "0.2", "--ppo-target-kl", "0.01", "--ppo-kl-host-stop", "--cuda-graph"],
     "--ppo-kl-host-stop and --cuda-graph exclude each other"),
    (["--ppo-clip", "0.2", "--ppo-target-kl", "small"], "invalid float value"),
])
def test_refusals_say_why(monkeypatch, capsys, argv, message):
    train, seen = _patched(monkeypatch)
    with pytest.raises(SystemExit):
        train.main(["cached-thor"] + argv)
    assert message in capsys.readouterr().err
    assert not seen


def test_experiment_passes_them_on():
    import inspect

    from vnav import train
    from vnav.a2c import A2CTrainer
    exp = train.make_trainer("cached-thor", ppo_clip=0.2, ppo_target_kl=0.02, ppo_kl_host_stop=True)
    assert exp.ppo_target_kl == 0.02 and exp.ppo_kl_host_stop is True
    off = train.make_trainer("cached-thor")
    assert off.ppo_target_kl is None and off.ppo_kl_host_stop is False
    params = inspect.signature(A2CTrainer.__init__).parameters
    src = inspect.getsource(train.Experiment.create_trainer)
    for name in ("ppo_target_kl", "ppo_kl_host_stop"):
        assert "%s=self.%s" % (name, name) in src
        assert params[name].default == getattr(off, name)


def test_metric_segment_rides_last():
    from vnav.metrics import metric_layout
    assert metric_layout(ppo=True, ppo_kl=True) == {"base": (0, 9), "ppo": (9, 4), "ppo_kl": (13, 3)}
    full = metric_layout(True, True, True, True, True, True, True, True, ppo_kl=True)
    assert list(full)[-1] == "ppo_kl" and full["ppo_kl"] == (35, 3) and full["ppo"] == (31, 4)
    # off by default: every layout from before is unchanged, by position too
    assert metric_layout(True, True, True, True, True, True, True, True) == {k: v for k, v in full.items()
                                                                             if k != "ppo_kl"}
    assert metric_layout(ppo=True) == {"base": (0, 9), "ppo": (9, 4)}
