"""numpy restatement of urt_auto_exposure and urt_tonemap (include/urt.h "auto-exposure and tone mapping"): float32 with one rounding per
operation, integer operations on view(np.uint32), Python ints for the 64-bit part.  The GPU results are compared with these bit for bit."""
import numpy as np

F = np.float32
U = np.uint32
BINS = 256
LINEAR, REINHARD, ACES = 0, 1, 2
FRESH = {"exposure": 0.0, "target": 0.0, "counted": 0, "skipped": 0, "hist": np.zeros(BINS, U)}


def luminance(rgba):
    """Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b of (..., 4) float32 texels, flattened."""
    p = np.ascontiguousarray(rgba, dtype=F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return (F(0.2126) * p[:, 0] + F(0.7152) * p[:, 1]) + F(0.0722) * p[:, 2]


def luminance_bin(Y):
    """The bin of positive finite luminances: clamp((int)(bits(Y) >> 21) - 380, 0, 255)."""
    bits = np.ascontiguousarray(Y, dtype=F).view(U)
    return np.clip((bits >> U(21)).astype(np.int64) - 380, 0, BINS - 1)


def texel_with_luminance(bits):
    """An (r, g, 0, 1) texel whose luminance has exactly the given bit pattern (a positive normal float): g carries it to within two
    ulps from below, r the small rest — 0.2126f*r is within 1e-7 of that rest, far less than half an ulp of the sum."""
    T = np.array([bits], dtype=U).view(F)[0]
    g = F(np.float64(T) / np.float64(F(0.7152)))
    while F(0.7152) * g > T:
        g = np.nextafter(g, F(0.0))
    rest = np.float64(T) - np.float64(F(0.7152) * g)
    px = np.array([F(rest / np.float64(F(0.2126))), g, 0.0, 1.0], dtype=F)
    assert luminance(px).view(U)[0] == bits, hex(bits)
    return px


def luminance_histogram_ref(rgba, count=None):
    """(hist, counted, skipped): step 1 of urt_auto_exposure.  count: None or the (..., 4) count texture, whose .x is read."""
    Y = luminance(rgba)
    with np.errstate(all="ignore"):
        ok = np.isfinite(Y) & (Y > F(0.0))
        if count is not None:
            ok &= np.ascontiguousarray(count, dtype=F).reshape(-1, 4)[:, 0] > F(0.0)
    hist = np.bincount(luminance_bin(Y)[ok], minlength=BINS).astype(U)
    return hist, int(hist.sum(dtype=np.uint64)), int(Y.size - ok.sum())


def trimmed_bins(hist, low_permille=100, high_permille=950):
    """(kept, M): how many samples of each bin have a rank in [lo, hi), and hi - lo; Python ints."""
    T = sum(int(h) for h in hist)
    lo, hi = T * low_permille // 1000, T * high_permille // 1000
    kept, prefix = [], 0
    for h in hist:
        a, b = max(prefix, lo), min(prefix + int(h), hi)
        kept.append(max(b - a, 0))
        prefix += int(h)
    return kept, hi - lo


def metered_luminance(hist, low_permille=100, high_permille=950):
    """L of step 2, or None when the trimmed window is empty."""
    kept, M = trimmed_bins(hist, low_permille, high_permille)
    if M == 0:
        return None
    q = (sum(k * n for k, n in enumerate(kept)) * 256) // M
    return np.array([(380 << 21) + (q << 13) + (1 << 20)], dtype=U).view(F)[0]


def exposure_resolve_ref(hist, prev_exposure=0.0, prev_target=0.0, key=0.18, min_exposure=1.0 / 64.0, max_exposure=64.0, rate=1.0,
                         low_permille=100, high_permille=950):
    """(exposure, target) after step 2 of urt_auto_exposure, as float32."""
    prev, target = F(prev_exposure), F(prev_target)
    L = metered_luminance(hist, low_permille, high_permille)
    if L is None:
        return prev, target
    target = min(max(F(key) / L, F(min_exposure)), F(max_exposure))
    if not np.isfinite(prev) or not prev > F(0.0) or F(rate) >= F(1.0):
        return target, target
    return prev + (target - prev) * F(rate), target


def auto_exposure_ref(rgba, count=None, state=FRESH, **params):
    """One urt_auto_exposure call: the state after it, in the form Context.exposure_state returns."""
    hist, counted, skipped = luminance_histogram_ref(rgba, count)
    exposure, target = exposure_resolve_ref(hist, state["exposure"], state["target"], **params)
    return {"exposure": float(exposure), "target": float(target), "counted": counted, "skipped": skipped, "hist": hist}


def tonemap_curve(x, op=ACES, white=4.0):
    """The operator on x = c * e, float32 array: clamp, then the curve."""
    with np.errstate(all="ignore"):
        x = np.where(x > F(0.0), np.minimum(x, F(65504.0)), F(0.0)).astype(F)
        if op == LINEAR:
            return x
        if op == REINHARD:
            w2 = F(white) * F(white)
            return np.minimum((x * (F(1.0) + x / w2)) / (F(1.0) + x), F(1.0))
        if op == ACES:
            return np.minimum((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14)), F(1.0))
    raise ValueError(f"unknown op {op}")


def tonemap_ref(rgba, exposure=1.0, white=4.0, op=ACES, flags=0, state_exposure=None):
    """urt_tonemap: state_exposure None = no d_state, else the state's exposure (used when finite and > 0)."""
    src = np.ascontiguousarray(rgba, dtype=F)
    e = F(exposure)
    if state_exposure is not None:
        s = F(state_exposure)
        if np.isfinite(s) and s > F(0.0):
            with np.errstate(all="ignore"):
                e = s * e
    out = src.copy()                                   # alpha: the same bits
    with np.errstate(all="ignore"):
        out[..., :3] = tonemap_curve(src[..., :3] * e, op, white)
    return out
