"""CPU: the numpy restatement of urt_auto_exposure / urt_tonemap (tests/tonemap_ref.py) held to the contract of include/urt.h — where
the bins lie, what is skipped, what the trimmed window keeps, how far the metered luminance can be from the geometric mean, and what the
three operators do at the ends of the float range."""
import numpy as np
import pytest

from tonemap_ref import (ACES, BINS, F, LINEAR, REINHARD, U, auto_exposure_ref, exposure_resolve_ref, luminance, luminance_bin,
                         luminance_histogram_ref, metered_luminance, texel_with_luminance, tonemap_curve, tonemap_ref, trimmed_bins)

OPS = (LINEAR, REINHARD, ACES)


def test_one_lands_in_bin_128_and_middle_grey_in_117():
    assert luminance_bin(F(1.0)) == 128 and luminance_bin(F(0.18)) == 117
    assert luminance_bin(F(2.0)) == 132 and luminance_bin(F(0.5)) == 124           # four bins per stop
    assert luminance_bin(F(2.0 ** -32)) == 0 and luminance_bin(np.nextafter(F(2.0 ** 32), F(0.0))) == 255
    assert luminance_bin(F(1e-45)) == 0 and luminance_bin(F(3e38)) == 255           # both clamps
    for bits, k in ((0x3F800000, 128), (F(0.18).view(U), 117)):
        hist, counted, skipped = luminance_histogram_ref(texel_with_luminance(int(bits)))
        assert hist[k] == 1 and counted == 1 and skipped == 0


def test_every_bin_edge_separates_its_two_neighbours():
    edges = np.arange(381, 380 + BINS, dtype=np.int64) << 21                        # the first float of bins 1 .. 255
    assert np.array_equal(luminance_bin(edges.astype(U).view(F)), np.arange(1, BINS))
    assert np.array_equal(luminance_bin((edges - 1).astype(U).view(F)), np.arange(0, BINS - 1))
    # the same through the luminance of a texel, at every edge
    px = np.stack([texel_with_luminance(int(b) - d) for b in edges for d in (0, 1)])
    hist, counted, skipped = luminance_histogram_ref(px)
    expect = np.ones(BINS, U) * 2
    expect[0] = expect[BINS - 1] = 1
    assert np.array_equal(hist, expect) and counted == 2 * (BINS - 1) and skipped == 0


def test_every_skip_class_is_counted():
    nan, inf = F(np.nan), F(np.inf)
    px = np.array([[1, 1, 1, 1],                     # counted
                   [nan, 1, 1, 1], [1, nan, 1, 1], [1, 1, nan, 1],      # NaN in any colour channel
                   [inf, 0, 0, 1], [0, -inf, 0, 1], [inf, -inf, 0, 1],  # infinite and inf - inf
                   [0, 0, 0, 1], [-0.0, -0.0, -0.0, 1], [-1, -1, -1, 1], [1, -2, 0, 1],   # not > 0
                   [inf, inf, inf, 1],               # an infinite luminance
                   [1e-45, 0, 0, 1],                 # 0.2126 * the smallest denormal rounds to 0
                   [1, 1, 1, nan],                   # alpha is not read
                   [1e-40, 1e-40, 1e-40, 1]], dtype=F)                  # a denormal luminance counts, in bin 0
    hist, counted, skipped = luminance_histogram_ref(px.reshape(3, 5, 4))
    assert counted == 3 and skipped == 12 and counted + skipped == 15
    assert hist[0] == 1 and hist.sum() == 3
    # with a count texture: zeros, negatives and NaN skip a texel that would count; a texel skipped twice is counted once
    cnt = np.zeros((15, 4), F)
    cnt[:, 0] = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, np.nan, -3]
    cnt[:, 1:] = nan                                                    # only .x is read
    hist, counted, skipped = luminance_histogram_ref(px, cnt)
    assert counted == 0 and skipped == 15 and not hist.any()
    cnt[:, 0] = [5e-45, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, inf, 1]
    hist, counted, skipped = luminance_histogram_ref(px, cnt)
    assert counted == 3 and skipped == 12


@pytest.mark.parametrize("seed", range(6))
def test_trimming_agrees_with_a_sort(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    Y = np.exp2(rng.uniform(-6, 6, n)).astype(F)
    px = np.zeros((n, 4), F)
    px[:, 1] = Y
    hist, counted, _ = luminance_histogram_ref(px)
    assert counted == n
    for low, high in ((0, 1000), (100, 950), (0, 1), (999, 1000), (500, 501), (250, 750), (int(rng.integers(0, 500)), int(rng.integers(500, 1001)))):
        ranked = np.sort(luminance_bin(luminance(px)))                 # ascending bin order; ties are interchangeable
        lo, hi = n * low // 1000, n * high // 1000
        kept, M = trimmed_bins(hist, low, high)
        assert M == hi - lo and sum(kept) == M
        assert np.array_equal(kept, np.bincount(ranked[lo:hi], minlength=BINS))
        L = metered_luminance(hist, low, high)
        if M == 0:
            assert L is None
            e, t = exposure_resolve_ref(hist, 0.7, 0.9, low_permille=low, high_permille=high)
            assert (e, t) == (F(0.7), F(0.9))                          # left as they are
        else:
            q = int(ranked[lo:hi].sum()) * 256 // M
            assert L.view(U) == (380 << 21) + (q << 13) + (1 << 20)


def test_metered_luminance_of_one_bin_is_its_centre():
    for k in (0, 1, 117, 128, 255):
        hist = np.zeros(BINS, U)
        hist[k] = 7
        first = np.array([(380 + k) << 21], U).view(F)[0]
        nxt = np.array([(381 + k) << 21], U).view(F)[0] if k < 255 else F(np.inf)
        L = metered_luminance(hist, 0, 1000)
        assert first < L < nxt and L.view(U) == ((380 + k) << 21) + (1 << 20)


@pytest.mark.parametrize("stops", (10, 16, 40))
def test_metered_luminance_is_within_a_quarter_stop_of_the_geometric_mean(stops):
    """The bound is derived: a sample lies anywhere in its quarter-stop bin while L reads the bin's centre (at most 1/8 stop each way per
    sample, 1/4 bin over the mean at the very worst), reading log2 piecewise-linearly in bit space errs by at most 0.0861 stop, and q is
    floored to 1/256 bin (0.001 stop): less than 0.25 stop in all."""
    rng = np.random.default_rng(stops)
    logs = rng.uniform(-stops / 2, stops / 2, 20000)
    px = np.zeros((logs.size, 4), F)
    px[:, 1] = np.exp2(logs) / 0.7152
    Y = luminance(px).astype(np.float64)
    hist, counted, _ = luminance_histogram_ref(px)
    assert counted == logs.size
    L = metered_luminance(hist, 0, 1000)
    assert abs(np.log2(np.float64(L)) - np.log2(Y).mean()) <= 0.25


def test_exposure_follows_the_target():
    hist = np.zeros(BINS, U)
    hist[128] = 100
    L = metered_luminance(hist)
    e, t = exposure_resolve_ref(hist)                                   # fresh: snaps
    assert e == t == F(0.18) / L
    for prev in (0.0, -1.0, np.nan, np.inf):                            # unusable: snaps
        assert exposure_resolve_ref(hist, prev, 0.0, rate=0.25)[0] == t
    e2, t2 = exposure_resolve_ref(hist, 1.0, 0.0, rate=0.25)
    assert t2 == t and e2 == F(1.0) + (t - F(1.0)) * F(0.25)
    assert exposure_resolve_ref(hist, 1.0, 0.0, rate=1.0)[0] == t and exposure_resolve_ref(hist, 1.0, 0.0, rate=np.inf)[0] == t
    assert exposure_resolve_ref(hist, min_exposure=1.0, max_exposure=2.0)[1] == F(1.0)
    assert exposure_resolve_ref(hist, max_exposure=0.125)[1] == F(0.125)
    s = auto_exposure_ref(np.zeros((2, 2, 4), F), state={"exposure": 0.5, "target": 0.25, "counted": 9, "skipped": 9, "hist": hist})
    assert (s["exposure"], s["target"], s["counted"], s["skipped"]) == (0.5, 0.25, 0, 4) and not s["hist"].any()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("white", (0.01, 1.0, 4.0, 65504.0))
def test_operators_are_monotone_start_at_zero_and_stay_in_range(op, white):
    x = np.concatenate([[0.0], np.exp2(np.linspace(-149, 16, 6000)), [65504.0]]).astype(F)
    x = np.unique(x)
    y = tonemap_curve(x, op, white)
    assert y.dtype == F and y[0] == 0 and np.all(np.diff(y) >= 0)
    assert np.all(y >= 0) and np.all(y <= (F(65504.0) if op == LINEAR else F(1.0)))
    if op != LINEAR:
        assert y[-1] == 1.0


@pytest.mark.parametrize("op", OPS)
def test_special_channels(op):
    nan, inf = F(np.nan), F(np.inf)
    top = tonemap_curve(np.array([65504.0], F), op)[0]
    assert top == (F(65504.0) if op == LINEAR else F(1.0))
    alpha = np.array([0x7FC00001, 0xFFFFFFFF, 0x80000000, 0x7F800000, 0x00000001, 0x3F800000], U).view(F)
    px = np.array([[nan, -1.0, inf], [-inf, -0.0, 0.0], [1e-45, 70000.0, 3e38], [-1e-45, 0.5, 2.0], [nan, nan, nan], [inf, inf, inf]], F)
    src = np.concatenate([px, alpha[:, None]], axis=1)
    out = tonemap_ref(src, op=op)
    y = lambda v: tonemap_curve(np.array([v], F), op)[0]               # noqa: E731
    expect = np.array([[0, 0, top], [0, 0, 0], [y(1e-45), top, top], [0, y(0.5), y(2.0)], [0, 0, 0], [top, top, top]], F)
    assert np.array_equal(out[:, :3].view(U), expect.view(U))
    assert np.array_equal(out[:, 3].view(U), alpha.view(U))             # bit for bit, NaN payloads included
    # the state's exposure multiplies params'; an unusable one is ignored
    a = tonemap_ref(src, exposure=0.5, op=op, state_exposure=4.0)
    assert np.array_equal(a.view(U), tonemap_ref(src, exposure=2.0, op=op).view(U))
    for s in (0.0, -2.0, np.nan, np.inf, -np.inf):
        assert np.array_equal(tonemap_ref(src, exposure=0.5, op=op, state_exposure=s).view(U), tonemap_ref(src, exposure=0.5, op=op).view(U))
