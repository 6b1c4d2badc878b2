"""The kink-free draw of tests/test_gpu_backward_replicas.py (tests/util.py: kinkfree_core_inputs), without a GPU: for every width set and row
count that module uses with a relu FeedForward, no hidden pre-activation z1 = W1 . gn2(x_row) + b1 is left within 10 . 1e-5 . S of zero
(S = |gn2(x)| . |W1|^T + |b1|), the redrawing ends well inside its 20 rounds, and the inputs stay what the other tests draw: fp32 in [0, 1)."""
import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import util as U

# (dims, R, E, N, G): the relu cases of the GPU module
SHAPES = [((64, 64, 64), 3, 1500, 400, 1), ((128, 64, 32), 3, 1500, 400, 1), ((16, 8, 16), 70, 50, 24, 1), ((16, 8, 16), 1, 300, 500, 70),
          ((10, 5, 3), 3, 1500, 400, 1), ((3, 4, 5), 3, 1500, 400, 1), ((64, 32, 16), 2, 1500, 400, 1)]
# the share of rows the first draw puts within the margin, measured once per width of the edge rows and rounded up: a helper that redraws
# nothing (or everything) is caught by the window
FIRST_SHARE = {128: (0.10, 0.40), 64: (0.03, 0.20), 16: (0.001, 0.05), 10: (0.0005, 0.02), 3: (0.0, 0.01)}


@pytest.mark.parametrize("eps_mode", [0, 1])
@pytest.mark.parametrize("dims,R,E,N,G", SHAPES, ids=[f"{'x'.join(map(str, s[0]))}-R{s[1]}-G{s[4]}" for s in SHAPES])
def test_no_row_is_left_within_the_margin(dims, R, E, N, G, eps_mode):
    rng = np.random.default_rng(7)
    p = O.make_core_params(rng, dims, eps_mode=eps_mode)
    xs, rounds, share = U.kinkfree_core_inputs(rng, p, R, E, N, G)
    assert rounds <= 10, rounds  # (20 is the limit; at most 7 were ever needed at these widths)
    lo, hi = FIRST_SHARE[dims[0]]
    assert lo <= share <= hi, share
    for t, x, T, d in zip("eng", xs, (E, N, G), dims):
        assert x.dtype == np.float32 and x.shape == (R, T, d)
        assert float(x.min()) >= 0.0 and float(x.max()) < 1.0
        assert not U.relu_kink_rows(p, t, x).any()
        # the condition itself, restated: every |z1| above the margin
        z = O.layernorm(x.astype(np.float64), p[f"ln2_{t}_gamma"], p[f"ln2_{t}_beta"], p["eps"], eps_mode, axis=-1)
        W1, b1 = p[f"ff_{t}_W1"].astype(np.float64), p[f"ff_{t}_b1"].astype(np.float64)
        S = np.abs(z) @ np.abs(W1).T + np.abs(b1)
        assert (np.abs(z @ W1.T + b1) > 10 * 1e-5 * S).all()


def test_a_row_on_the_kink_is_reported_and_redrawn():
    """a bias that puts one hidden unit of one row exactly on zero: the row is reported, and the redraw moves it"""
    rng = np.random.default_rng(8)
    p = O.make_core_params(rng, (10, 5, 3))
    x = rng.random((2, 7, 5), dtype=np.float32)
    z = O.layernorm(x.astype(np.float64), p["ln2_n_gamma"], p["ln2_n_beta"], p["eps"], 0, axis=-1)
    p["ff_n_b1"] = p["ff_n_b1"].copy()
    p["ff_n_b1"][3] = np.float32(-(z[1, 4] @ p["ff_n_W1"][3].astype(np.float64)))
    bad = U.relu_kink_rows(p, "n", x)
    assert bad[1, 4]
    xs, rounds, _ = U.kinkfree_core_inputs(np.random.default_rng(9), p, 2, 11, 7, 1)
    assert not any(U.relu_kink_rows(p, t, v).any() for t, v in zip("eng", xs))


def test_the_round_limit_fails_the_draw():
    """a FeedForward whose every pre-activation is zero has no kink-free row: the helper gives up with an AssertionError, it does not return"""
    p = O.make_core_params(np.random.default_rng(10), (3, 4, 5))
    for t in "eng":
        p[f"ff_{t}_W1"] = np.zeros_like(p[f"ff_{t}_W1"]); p[f"ff_{t}_b1"] = np.zeros_like(p[f"ff_{t}_b1"])
    with pytest.raises(AssertionError, match="after 3 rounds"):
        U.kinkfree_core_inputs(np.random.default_rng(11), p, 1, 5, 4, 1, max_rounds=3)
