"""--image-size on the vnav.train command line, and training straight from a 300x400 scene
file with the frames resized on the device (no offline conversion)."""
import numpy as np
import pytest


def test_image_size_reaches_the_env_kwargs(monkeypatch):
    from vnav import train
    seen = {}

    class Exp:
        def run(self, resume=False):
            seen["ran"] = True

    def fake(name, env_kwargs=None, **kw):
        seen["name"], seen["env_kwargs"] = name, env_kwargs
        return Exp()

    monkeypatch.setattr(train, "make_trainer", fake)
    monkeypatch.setattr(train.vdist, "init_distributed", lambda: None)
    assert train.main(["cached-thor", "--scene", "a.npz", "--scene", "b.h5", "--image-size", "84", "84"]) == 0
    assert seen["ran"] and seen["env_kwargs"] == dict(scenes=["a.npz", "b.h5"], image_size=(84, 84))
    assert train.main(["thor-cached-auxiliary", "--scene", "grid.pkl", "--image-size", "174", "174"]) == 0
    assert seen["env_kwargs"] == dict(scene="grid.pkl", image_size=(174, 174))
    assert train.main(["cached-thor", "--scene", "a.npz"]) == 0
    assert seen["env_kwargs"] == dict(scenes=["a.npz"])


@pytest.mark.gpu
def test_trains_from_a_300x400_scene_file(golden, tmp_path):
    import resize_ref as rr
    from vnav import train
    d = golden("ingest.npz")
    frames = np.random.RandomState(0).randint(0, 256, size=(8, 300, 400, 3)).astype(np.uint8)
    path = str(tmp_path / "dump.npz")
    np.savez(path, graph=d["r_graph"], shortest_path_distance=d["r_spd"], observation=frames)
    exp = train.make_trainer("cached-thor", env_kwargs=dict(scenes=[path], image_size=(84, 84), num_envs=8),
                             save_dir=str(tmp_path), max_time_steps=8 * 20 * 2, saving_period=0,
                             episode_log_interval=0, logger=None)
    m = exp.run()
    assert m["step"] == 320 and m["updates"] == 2 and np.isfinite(m["loss"])
    env = exp.env
    assert env.frame_shape == (84, 84, 3)
    assert np.array_equal(env.scenes[0].observations, rr.resize(frames, (84, 84)))
