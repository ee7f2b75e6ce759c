"""The numpy restatement of urt_skin_vertices / urt_buffer_bounds (tests/skin_ref.py) against float64 skinning and on hand-made cases.
No GPU: tests/test_gpu_skin.py holds the library to the restatement bit for bit."""
import numpy as np

import skin_ref as S

F = np.float32


def random_case(n=500, n_bones=7, seed=0):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-3, 3, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3)).astype(F)
    j = rng.integers(0, n_bones, (n, 4)).astype(np.int32)
    w = rng.uniform(0, 1, (n, 4)).astype(F)
    w = (w / w.sum(axis=1, keepdims=True)).astype(F)
    A = rng.uniform(-1.5, 1.5, (n_bones, 12)).astype(F)
    return P, N, j, w, A


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_fma_is_exact_on_a_case_double_rounding_gets_wrong():
    # a * b = 1 + 2^-24 + 2^-48 exactly (a tie broken upwards by the last bit); c = 0: plain float64 -> float32 rounding would be fine, the
    # sum with c = 2^-60 is where the float64 sum rounds the sticky bit away
    a, b = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12)                                  # product 1 + 2^-11 + 2^-24: a tie for float32
    assert S.fma32(a, b, F(2.0 ** -60)) == F(1 + 2.0 ** -11 + 2.0 ** -23)        # just above the tie: up
    assert S.fma32(a, b, F(-2.0 ** -60)) == F(1 + 2.0 ** -11)                    # just below: down
    assert np.isinf(S.fma32(F(3e38), F(10), F(0))) and np.isnan(S.fma32(F(np.inf), F(0), F(1)))


def test_against_float64_within_the_derived_bound():
    for seed, n_bones in ((0, 7), (1, 1), (2, 300)):
        P, N, j, w, A = random_case(seed=seed, n_bones=n_bones)
        w[::7] *= F(-1.7)                                                        # weights are not normalised, and may be negative
        got, _ = S.skin(P, N, j, w, A)
        want, bound = S.skin64(P, j, w, A)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert err.max() > 0                                                     # (float32 does round: the bound is not vacuous)


def test_single_live_bone_of_weight_one_is_the_affine_map_bit_for_bit():
    P, N, j, w, A = random_case()
    w[:] = 0
    w[:, 2] = 1                                                                  # the third term carries everything
    got, _ = S.skin(P, N, j, w, A)
    a = A[j[:, 2]]
    want = ((a[:, 0:3] * P[:, 0:1] + a[:, 3:6] * P[:, 1:2]) + a[:, 6:9] * P[:, 2:3]) + a[:, 9:12]
    assert np.array_equal(bits(got), bits(want))


def test_terms_that_are_not_live_add_nothing():
    P, N, j, w, A = random_case()
    ref_v, ref_n = S.skin(P, N, j, w, A)
    # a zero weight with an index of 10^9 (or a negative one) leaves the result unchanged
    j2, w2 = j.copy(), w.copy()
    w2[:, 3] = 0
    base_v, base_n = S.skin(P, N, j2, w2, A)
    for wild in (10 ** 9, -1, -2 ** 31, len(A)):
        j3 = j2.copy(); j3[:, 3] = wild
        v, n = S.skin(P, N, j3, w2, A)
        assert np.array_equal(bits(v), bits(base_v)) and np.array_equal(bits(n), bits(base_n)), wild
    # an index out of range with a non-zero weight is skipped: the same as a zero weight
    for wild in (10 ** 9, -1, len(A)):
        j3 = j.copy(); j3[:, 3] = wild
        v, n = S.skin(P, N, j3, w, A)
        assert np.array_equal(bits(v), bits(base_v)) and np.array_equal(bits(n), bits(base_n)), wild
    assert not np.array_equal(bits(ref_v), bits(base_v))
    # all four dead: +0.0 exactly, and the normal (L2 == 0) stays the zero vector
    v, n = S.skin(P, N, j, np.zeros_like(w), A)
    assert not bits(v).any() and not bits(n).any()
    # a NaN weight is live
    w4 = w.copy(); w4[5, 1] = np.nan
    v, n = S.skin(P, N, j, w4, A)
    assert np.isnan(v[5]).all() and np.isnan(n[5]).all() and np.array_equal(bits(np.delete(v, 5, 0)), bits(np.delete(ref_v, 5, 0)))


def test_the_normal_rule_at_zero_inf_and_nan():
    ident = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)
    j = np.zeros((5, 4), np.int32)
    w = np.zeros((5, 4), F); w[:, 0] = 1
    P = np.zeros((5, 3), F)
    N = np.array([[0, 0, 0], [3, 0, 4], [1e30, 1e30, 0], [np.nan, 1, 0], [1e-30, 0, 0]], F)
    _, n = S.skin(P, N, j, w, ident)
    assert not bits(n[0]).any()                                                  # L2 == 0: s as it is, not NaN
    assert np.array_equal(bits(n[1]), bits(np.array([3, 0, 4], F) * (F(1) / np.sqrt(F(25)))))
    assert np.array_equal(bits(n[2]), bits(N[2]))                                # L2 overflows to inf: s as it is
    assert np.isnan(n[3]).all()                                                  # 0 * NaN: every component, and L2, is NaN: s as it is
    assert np.array_equal(bits(n[4]), bits(N[4]))                                # L2 underflows to 0: s as it is
    # without normals nothing is returned for them
    assert S.skin(P, None, j, w, ident)[1] is None


def test_bounds_ignore_elements_that_are_not_finite():
    v = np.array([[1, 2, 3], [np.nan, -100, 100], [-1, 5, 0], [0, np.inf, 0], [4, -2, -0.0], [0, 0, -np.inf]], F)
    lo, hi, n = S.bounds(v)
    assert n == 3 and lo.tolist() == [-1, -2, 0] and hi.tolist() == [4, 5, 3]
    lo, hi, n = S.bounds(v, 1, 1)
    assert n == 0 and np.isposinf(lo).all() and np.isneginf(hi).all()
    lo, hi, n = S.bounds(v, 2, 3)
    assert n == 2 and lo.tolist() == [-1, -2, 0] and hi.tolist() == [4, 5, 0]


def test_two_bone_bend_is_a_rigid_rotation_at_the_top_and_the_identity_at_the_bottom():
    from unityraytracer_amd import scenes
    v = scenes.uv_blob(12, 9)[0]
    idx, wgt, bones = S.two_bone_bend(v, 35.0)
    out, _ = S.skin(v, None, idx, wgt, bones)
    bottom, top = int(np.argmin(v[:, 1])), int(np.argmax(v[:, 1]))
    assert np.array_equal(bits(out[bottom]), bits(v[bottom] * F(1) + F(0)))
    centre = v.mean(axis=0)
    assert abs(np.linalg.norm(out[top] - centre) - np.linalg.norm(v[top] - centre)) < 1e-5
    assert np.abs(out - v).max() > 0.1
