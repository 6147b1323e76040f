"""image_size through the public surface on the GPU: vnav.make / VectorEnv, CachedThorEnv,
load_npz and resize_scene, against tests/resize_ref.py on the 8-state 100x100 cached scene of
tests/golden/ingest.npz."""
import numpy as np
import pytest
import torch

import resize_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def raw(golden):
    d = golden("ingest.npz")
    return d["r_graph"], d["r_spd"], d["r_frames"]


@pytest.fixture(scope="module")
def want84(raw):
    return rr.resize(raw[2], (84, 84))


def test_make_with_image_size_emits_resized_frames(raw, want84):
    import vnav
    scene = vnav.scene_from_arrays(*raw)
    assert scene.frame_shape == (100, 100, 3)
    env = vnav.make("CachedThor-v0", scene, 4, seed=5, max_episode_steps=7, image_size=(84, 84))
    assert env.frame_shape == (84, 84, 3) and env.obs_shape == (84, 84, 3)
    assert scene.frame_shape == (100, 100, 3) and scene.observations.shape == (8, 100, 100, 3)  # not edited
    assert env.scenes[0].graph is scene.graph and env.scenes[0].spd is scene.spd  # tables shared
    img, goal = env.reset()
    assert tuple(img.shape) == (4, 84, 84, 3) and img.dtype == torch.uint8
    rng = np.random.RandomState(0)
    dones = 0
    for t in range(50):
        a = torch.as_tensor(rng.randint(0, 4, size=4).astype(np.int32), device="cuda")
        (img, goal), reward, done, info = env.step(a)
        rows, grows = info["img_row"].cpu().numpy(), info["goal_row"].cpu().numpy()
        st = env.get_state().cpu().numpy()
        # one scene: arena row = state index. A finished env re-emits its last observation
        # (cached.py:90-96) while its record already holds the next episode
        live = ~done.cpu().numpy()
        assert np.array_equal(grows[live], st[2][live]), t
        assert np.array_equal(rows[live], info["state"].cpu().numpy()[live]), t
        assert np.array_equal(img.cpu().numpy(), want84[rows]), t
        assert np.array_equal(goal.cpu().numpy(), want84[grows]), t
        dones += int(done.sum())
    assert dones > 0 and env.error_flags() == 0


def test_image_size_of_the_scene_changes_nothing(raw):
    import vnav
    scene = vnav.scene_from_arrays(*raw)
    a_env = vnav.make("CachedThor-v0", scene, 4, seed=9, max_episode_steps=11)
    b_env = vnav.make("CachedThor-v0", scene, 4, seed=9, max_episode_steps=11, image_size=(100, 100))
    assert b_env.scenes[0] is scene and b_env.frame_shape == (100, 100, 3)
    for x, y in zip(a_env.reset(), b_env.reset()):
        assert torch.equal(x, y)
    rng = np.random.RandomState(1)
    for t in range(20):
        a = torch.as_tensor(rng.randint(0, 4, size=4).astype(np.int32), device="cuda")
        (ia, ga), ra, da, fa = a_env.step(a)
        (ib, gb), rb, db, fb = b_env.step(a)
        assert torch.equal(ia, ib) and torch.equal(ga, gb) and torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(fa["state"], fb["state"]), t
    # a synthetic scene of that size passes through too; at another size it cannot be resized
    syn = vnav.synthetic_scene(0)
    assert vnav.VectorEnv([syn], 2, image_size=(84, 84)).scenes[0] is syn
    with pytest.raises(ValueError):
        vnav.VectorEnv([syn], 2, image_size=(42, 42))
    with pytest.raises(ValueError):
        vnav.resize_scene(syn, (42, 42))


def test_load_npz_with_image_size(raw, want84, tmp_path):
    import vnav
    path = str(tmp_path / "scene.npz")
    np.savez(path, graph=raw[0], shortest_path_distance=raw[1], observation=raw[2])
    a = vnav.load_npz(path, image_size=(84, 84))
    b = vnav.resize_scene(vnav.load_npz(path), (84, 84))
    assert a.frame_shape == b.frame_shape == (84, 84, 3)
    assert np.array_equal(a.observations, b.observations) and np.array_equal(a.observations, want84)
    assert np.array_equal(a.graph, b.graph) and np.array_equal(a.spd, b.spd)
    assert vnav.load_npz(path, image_size=(100, 100)).frame_shape == (100, 100, 3)


def test_resize_scene_resizes_every_frame_set(raw):
    import vnav
    from vnav.scenes import Scene
    rng = np.random.RandomState(2)
    comp = rng.randint(0, 256, size=raw[2].shape).astype(np.uint8)
    depth = rng.randint(0, 256, size=raw[2].shape[:3] + (1,)).astype(np.uint8)
    seg = rng.randint(0, 256, size=raw[2].shape).astype(np.uint8)
    scene = Scene(graph=raw[0], spd=raw[1], frame_shape=(100, 100, 3), observations=raw[2], companion=comp,
                  depth=depth, segmentation=seg, goals=[3], name="all")
    out = vnav.resize_scene(scene, (50, 42))
    assert out.frame_shape == (50, 42, 3) and out.goals == [3] and out.name == "all"
    assert out.graph is scene.graph and out.spd is scene.spd
    for k in ("observations", "companion", "depth", "segmentation"):
        assert np.array_equal(getattr(out, k), rr.resize(getattr(scene, k), (50, 42))), k


def test_cached_thor_env_image_size(raw, want84):
    import vnav
    env = vnav.CachedThorEnv(vnav.scene_from_arrays(*raw), seed=1, image_size=(84, 84))
    img, goal = env.reset()
    s, g = env.state
    assert img.shape == (84, 84, 3) and img.dtype == np.float64
    assert np.array_equal(img, want84[s].astype(np.float64) / 255.0)
    assert np.array_equal(goal, want84[g].astype(np.float64) / 255.0)
    env.close()
