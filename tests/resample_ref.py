"""numpy float32 restatements of the resampling entry points (include/urt.h "resampling"): urt_select_pixels and urt_blend_samples.
Every operation is float32 with one rounding, in the order the header states."""
import numpy as np

F = np.float32


def select_pixels_ref(count, below):
    """The (n, 2) int32 list of (x, y) urt_select_pixels writes for a count image (h, w, 4) or (h, w) float32: the pixels with
    !(count.x >= below) in ascending texel index y * w + x."""
    c = np.asarray(count, F)
    if c.ndim == 3:
        c = c[..., 0]
    with np.errstate(invalid="ignore"):
        selected = ~(c >= F(below))                                  # NaN fails the comparison: selected
    ys, xs = np.nonzero(selected)                                    # row-major: ascending y * w + x
    return np.stack([xs, ys], axis=1).astype(np.int32)


def blend_samples_ref(xy, samples, dst, count, weight=1.0, max_history=0.0):
    """(dst, count) after urt_blend_samples(xy, samples, n, weight, dst, count, max_history) on (h, w, 4) float32 images; xy (n, 2)
    int32 with distinct pixels, samples (n, 4) float32.  A pixel outside the image is skipped."""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    t = np.asarray(samples, F).reshape(-1, 4)
    out, cnt = np.array(dst, F), np.array(count, F)
    h, w = out.shape[:2]
    inside = (xy[:, 0] >= 0) & (xy[:, 0] < w) & (xy[:, 1] >= 0) & (xy[:, 1] < h)
    x, y, t = xy[inside, 0], xy[inside, 1], t[inside]
    assert len(set(zip(x.tolist(), y.tolist()))) == len(x), "the pixels of a list must be distinct"
    wt, mh = F(weight), F(max_history)
    c, n = out[y, x], cnt[y, x, 0]
    with np.errstate(all="ignore"):
        capped = np.fmin(n, np.fmax(mh - wt, F(0.0))) if mh > F(0) else n
        s = np.where(~np.isfinite(n) | (n < F(0)), F(0), capped).astype(F)
        a = wt / (s + wt)
        ia = F(1.0) - a
        new = np.empty_like(c)
        for ch in range(3):
            new[:, ch] = t[:, ch] * a + c[:, ch] * ia
        new[:, 3] = a * a + c[:, 3] * ia
        out[y, x] = new
        cnt[y, x] = 0
        cnt[y, x, 0] = s + wt
    return out, cnt
