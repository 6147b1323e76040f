"""vnav.metrics.metric_layout: the segments of A2CTrainer's metric vector (step(sync=False)["raw"])
for all 32 flag combinations against literal offsets. No GPU, and the native library is not loaded."""
import itertools

import pytest

FLAGS = ("unreal", "nav_metrics", "expert", "geo_curriculum", "shaping")

# (unreal, nav_metrics, expert, geo_curriculum, shaping) -> ({segment: (offset, width)}, total width)
EXPECTED = {
    (0, 0, 0, 0, 0): ({"base": (0, 9)}, 9),
    (0, 0, 0, 0, 1): ({"base": (0, 9), "shaping": (9, 3)}, 12),
    (0, 0, 0, 1, 0): ({"base": (0, 9), "curriculum": (9, 1)}, 10),
    (0, 0, 0, 1, 1): ({"base": (0, 9), "curriculum": (9, 1), "shaping": (10, 3)}, 13),
    (0, 0, 1, 0, 0): ({"base": (0, 9), "expert": (9, 4)}, 13),
    (0, 0, 1, 0, 1): ({"base": (0, 9), "expert": (9, 4), "shaping": (13, 3)}, 16),
    (0, 0, 1, 1, 0): ({"base": (0, 9), "expert": (9, 4), "curriculum": (13, 1)}, 14),
    (0, 0, 1, 1, 1): ({"base": (0, 9), "expert": (9, 4), "curriculum": (13, 1), "shaping": (14, 3)}, 17),
    (0, 1, 0, 0, 0): ({"base": (0, 9), "nav": (9, 4)}, 13),
    (0, 1, 0, 0, 1): ({"base": (0, 9), "nav": (9, 4), "shaping": (13, 3)}, 16),
    (0, 1, 0, 1, 0): ({"base": (0, 9), "nav": (9, 4), "curriculum": (13, 1)}, 14),
    (0, 1, 0, 1, 1): ({"base": (0, 9), "nav": (9, 4), "curriculum": (13, 1), "shaping": (14, 3)}, 17),
    (0, 1, 1, 0, 0): ({"base": (0, 9), "nav": (9, 4), "expert": (13, 4)}, 17),
    (0, 1, 1, 0, 1): ({"base": (0, 9), "nav": (9, 4), "expert": (13, 4), "shaping": (17, 3)}, 20),
    (0, 1, 1, 1, 0): ({"base": (0, 9), "nav": (9, 4), "expert": (13, 4), "curriculum": (17, 1)}, 18),
    (0, 1, 1, 1, 1): ({"base": (0, 9), "nav": (9, 4), "expert": (13, 4), "curriculum": (17, 1), "shaping": (18, 3)},
                      21),
    (1, 0, 0, 0, 0): ({"base": (0, 12)}, 12),
    (1, 0, 0, 0, 1): ({"base": (0, 12), "shaping": (12, 3)}, 15),
    (1, 0, 0, 1, 0): ({"base": (0, 12), "curriculum": (12, 1)}, 13),
    (1, 0, 0, 1, 1): ({"base": (0, 12), "curriculum": (12, 1), "shaping": (13, 3)}, 16),
    (1, 0, 1, 0, 0): ({"base": (0, 12), "expert": (12, 4)}, 16),
    (1, 0, 1, 0, 1): ({"base": (0, 12), "expert": (12, 4), "shaping": (16, 3)}, 19),
    (1, 0, 1, 1, 0): ({"base": (0, 12), "expert": (12, 4), "curriculum": (16, 1)}, 17),
    (1, 0, 1, 1, 1): ({"base": (0, 12), "expert": (12, 4), "curriculum": (16, 1), "shaping": (17, 3)}, 20),
    (1, 1, 0, 0, 0): ({"base": (0, 12), "nav": (12, 4)}, 16),
    (1, 1, 0, 0, 1): ({"base": (0, 12), "nav": (12, 4), "shaping": (16, 3)}, 19),
    (1, 1, 0, 1, 0): ({"base": (0, 12), "nav": (12, 4), "curriculum": (16, 1)}, 17),
    (1, 1, 0, 1, 1): ({"base": (0, 12), "nav": (12, 4), "curriculum": (16, 1), "shaping": (17, 3)}, 20),
    (1, 1, 1, 0, 0): ({"base": (0, 12), "nav": (12, 4), "expert": (16, 4)}, 20),
    (1, 1, 1, 0, 1): ({"base": (0, 12), "nav": (12, 4), "expert": (16, 4), "shaping": (20, 3)}, 23),
    (1, 1, 1, 1, 0): ({"base": (0, 12), "nav": (12, 4), "expert": (16, 4), "curriculum": (20, 1)}, 21),
    (1, 1, 1, 1, 1): ({"base": (0, 12), "nav": (12, 4), "expert": (16, 4), "curriculum": (20, 1),
                       "shaping": (21, 3)}, 24),
}


def test_expected_table_covers_every_combination():
    assert set(EXPECTED) == set(itertools.product((0, 1), repeat=len(FLAGS)))


@pytest.mark.parametrize("flags", sorted(EXPECTED))
def test_layout_equals_the_literal_table(flags):
    from vnav import metrics
    layout = metrics.metric_layout(**{k: bool(v) for k, v in zip(FLAGS, flags)})
    segments, width = EXPECTED[flags]
    assert layout == segments
    assert list(layout) == list(segments)  # and in the vector's order
    offset, last = list(layout.values())[-1]
    assert offset + last == width
    assert not {"torch", "ctypes", "_lib"} & set(vars(metrics))  # pure: nothing of the GPU or the library


def test_positional_order_is_the_trainers():
    """A2CTrainer passes the flags by position."""
    from vnav.metrics import metric_layout
    assert metric_layout(True, True, True, True, True) == EXPECTED[(1, 1, 1, 1, 1)][0]
    assert metric_layout(False, False, False, False, True) == EXPECTED[(0, 0, 0, 0, 1)][0]
    assert metric_layout(False, True) == EXPECTED[(0, 1, 0, 0, 0)][0]
