#!/usr/bin/env python3
"""Mine the reference's capture Screenshots/25.64697-62.png — a 1393 x 729 screenshot of Scene1.unity — for the silhouettes of its
objects: tests/golden/screenshot_silhouettes.json, NUMBERS only (spans, boxes, thresholds, measured differences); the image stays in
the reference.  Run by hand from the repository root, with the oracle built:

    python tests/golden/make_silhouette_fixtures.py [/root/reference]

What is segmented, all in fractions of the frame with rows counted from the top (tests/silhouette_ref.py has the conventions):

  Cube (1)    the black pentagon: mean RGB < 0.02, largest connected component, each row taken from its first to its last pixel (the single
              brighter pixels inside are path-tracing noise and break a row's run; checked: they are under 0.5 % of the area); its per-row spans, area,
              centroid and box.  It shows black because its material is a perfect mirror shaded with object-space normals (A.6).
  Capsule     green dominance, g > 1.5 max(r, b) and g > 0.1, in the upper right quarter of the frame; the box of every such pixel
              (the green is its outline's reflection: the area means nothing, the extremes are the capsule's).
  Cylinder    darker than the sky: mean RGB < 0.25 in the upper left quarter, largest component (the darkest clouds there are 0.33;
              the small chrome ball beside it, only in the capture, is a component of its own).
  Sphere (1)  its centre is level with the camera, so its upper half stands against the sky and its widest row is the horizon's:
              mean RGB < 0.30 (the sphere's 95th percentile is 0.295, the sky's 1st 0.37), largest component in a window that ends
              four rows above the horizon, where the sphere is 0.2 pixels narrower than at its widest.
  spheres     on the ground, bluer than it: b > 0.8 r below the horizon, largest component inside a window read off the capture.
              The chrome undersides take the ground's colour, so only top, left and right are mined.

Every threshold is swept by -20 % and +20 %; the spread of each edge over the sweep is recorded.  An edge of the cylinder or of a
sphere is kept when its extreme pixel lies inside the window it was segmented in at every step of the sweep (an edge on the window's
bound is the window's, not the object's), it is stable (spread <= STABLE of the frame) and within MAX_DIFFERENCE of the oracle's
render of the id scene (silhouette_ref.id_scene); its tolerance is twice that measured difference.  The others are listed under "dropped_edges" with their
figures.  The capsule's four edges carry the fixed tolerance 0.015, the cube the bounds of tests/test_reference_silhouettes.py."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

CAPTURE = "25.64697-62.png"
SWEEP = (0.8, 1.0, 1.2)
STABLE = 0.003                                                 # two rows of the 729: what one threshold step may move a kept edge
MAX_DIFFERENCE = 0.005                                         # twice this is the largest tolerance an edge may need
# windows (left, right, top, bottom) read off the capture by eye, each holding one sphere's visible upper part and no other sphere's
SPHERE_WINDOWS = {"Sphere (1)": (0.65, 0.82, 0.38, 0.495), "Sphere": (0.0, 0.25, 0.505, 0.75), "Sphere (6)": (0.60, 0.68, 0.505, 0.60),
                  "Sphere (7)": (0.792, 0.838, 0.53, 0.63), "Sphere (8)": (0.838, 0.96, 0.52, 0.67)}
WINDOWS = dict(SPHERE_WINDOWS, Capsule=(0.5, 1.0, 0.0, 0.5), Cylinder=(0.0, 0.5, 0.0, 0.5))       # the upper right and upper left quarters
NOT_IN_CAPTURE = [{"name": "Cube", "reason": "the 0.2-scale cube 1.3 units in front of the camera: its projected box x[0.058 0.169] y[0.256 0.395] "
                                             "shows sky in the capture (it was disabled or moved when the capture was taken)"}]
ONLY_IN_CAPTURE = [{"name": "Sphere (5)", "reason": "the pink emissive ball in mid-frame; its RayTraceObject is disabled in Scene1.unity"},
                   {"name": "Sphere (2)", "reason": "the small chrome ball above it; its RayTraceObject is disabled in Scene1.unity"}]


def largest_component(mask):
    from scipy import ndimage
    lab, n = ndimage.label(mask)
    if n == 0:
        return mask
    sizes = ndimage.sum(mask, lab, range(1, n + 1))
    return lab == 1 + int(np.argmax(sizes))


def window_pixels(box, w, h):
    """(x0, x1, y0, y1): the window holds columns x0 .. x1 - 1 and rows y0 .. y1 - 1."""
    return int(round(box[0] * w)), int(round(box[1] * w)), int(round(box[2] * h)), int(round(box[3] * h))


def window(mask, box):
    out = np.zeros_like(mask)
    x0, x1, y0, y1 = window_pixels(box, mask.shape[1], mask.shape[0])
    out[y0:y1, x0:x1] = mask[y0:y1, x0:x1]
    return out


def clipped_edges(mask, box):
    """The edges of a mask whose extreme pixel lies on the bound of the window it was segmented in: that edge is the window's, read off
    by eye, and not the object's."""
    x0, x1, y0, y1 = window_pixels(box, mask.shape[1], mask.shape[0])
    ys, xs = np.nonzero(mask)
    return {e for e, hit in (("left", xs.min() == x0), ("right", xs.max() == x1 - 1), ("top", ys.min() == y0), ("bottom", ys.max() == y1 - 1)) if hit}


def segment(a, name, scale):
    """The mask of one object in the capture `a` ((h, w, 3) in 0..1) with its threshold scaled by `scale`."""
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    if name == "Cube (1)":
        m = largest_component(a.mean(axis=2) < 0.02 * scale)
        first, last = np.argmax(m, axis=1), m.shape[1] - 1 - np.argmax(m[:, ::-1], axis=1)
        x = np.arange(m.shape[1])[None, :]                      # each row from its first to its last dark pixel: one run per row
        return m.any(axis=1)[:, None] & (x >= first[:, None]) & (x <= last[:, None])
    if name == "Capsule":
        return window((g > 1.5 * scale * np.maximum(r, b)) & (g > 0.1), WINDOWS[name])
    if name == "Cylinder":
        return largest_component(window(a.mean(axis=2) < 0.25 * scale, WINDOWS[name]))
    if name == "Sphere (1)":                                   # above the horizon, against the sky
        return largest_component(window(a.mean(axis=2) < 0.30 * scale, WINDOWS[name]))
    return largest_component(window(b > 0.8 * scale * r, WINDOWS[name]))


def mine(capture_path):
    from PIL import Image
    import silhouette_ref as S
    a = np.asarray(Image.open(capture_path).convert("RGB"), dtype=np.float64) / 255.0
    h, w = a.shape[:2]
    assert (w, h) == (S.WIDTH, S.HEIGHT)
    sc, ids = S.id_scene()
    _, ours = S.oracle_ids(sc, mode=1)
    r6 = lambda x: round(float(x), 6)
    out = {"capture": {"name": CAPTURE, "width": w, "height": h}, "sweep": list(SWEEP), "stable_spread": STABLE, "max_difference": MAX_DIFFERENCE,
           "objects": {}, "dropped_edges": [], "not_in_capture": NOT_IN_CAPTURE, "only_in_capture": ONLY_IN_CAPTURE}
    # Cube (1): spans, statistics, and the IoU with the oracle's mask over the sweep
    oracle_cube = ours == ids["Cube (1)"][0]
    masks = [segment(a, "Cube (1)", s) for s in SWEEP]
    cube = masks[1]
    noise = int(cube.sum() - (cube & (a.mean(axis=2) < 0.02)).sum())
    assert noise <= 0.005 * cube.sum(), f"Cube (1): {noise} of {int(cube.sum())} pixels inside the row spans are not dark"
    spans = []
    for row in np.nonzero(cube.any(axis=1))[0]:
        xs = np.nonzero(cube[row])[0]
        spans.append([int(row), int(xs[0]), int(xs[-1])])
    st = S.mask_stats(cube)
    ious = [S.iou(m, oracle_cube) for m in masks]
    moved = max(ious) - min(ious)
    out["objects"]["Cube (1)"] = {
        "rule": "mean RGB < 0.02, largest component, rows first to last", "noise_pixels_inside": noise, "area": r6(st["area"]), "centroid": [r6(c) for c in st["centroid"]],
        "box": {e: r6(v) for e, v in st["box"].items()}, "spans": spans,
        "iou_with_oracle": r6(ious[1]), "iou_with_oracle_over_sweep": [r6(i) for i in ious],
        # the sweep moves the IoU by less than 0.01: the bound stays 0.95; otherwise the swept minimum less 0.01
        "iou_bound": 0.95 if moved <= 0.01 else r6(min(ious) - 0.01)}
    for name in ["Capsule", "Cylinder"] + list(SPHERE_WINDOWS):
        masks = [segment(a, name, s) for s in SWEEP]
        boxes = [S.mask_stats(m)["box"] for m in masks]
        clipped = set().union(*(clipped_edges(m, WINDOWS[name]) for m in masks))      # in any step of the sweep
        theirs = S.mask_stats(ours == ids[name][0])["box"]
        edges = {}
        for e in S.EDGES:
            if name in SPHERE_WINDOWS and e == "bottom":
                continue
            vals = [bx[e] for bx in boxes]
            rec = {"value": r6(vals[1]), "oracle": r6(theirs[e]), "difference": r6(abs(vals[1] - theirs[e])), "spread_over_sweep": r6(max(vals) - min(vals))}
            if e in clipped:
                out["dropped_edges"].append(dict(rec, object=name, edge=e, reason="clipped by the window it was segmented in"))
                continue
            if name == "Capsule":
                rec["tolerance"] = 0.015
            else:
                why = []
                if rec["spread_over_sweep"] > STABLE:
                    why.append("unstable under the threshold sweep")
                if rec["difference"] > MAX_DIFFERENCE:
                    why.append("would need a tolerance above 0.01")
                if why:
                    out["dropped_edges"].append(dict(rec, object=name, edge=e, reason=" and ".join(why)))
                    continue
                rec["tolerance"] = r6(2 * rec["difference"])
            edges[e] = rec
        if edges:
            out["objects"][name] = {"edges": edges}
    return out


def reference_root():
    """Where the reference's tree is looked for: the first argument, else $URT_REFERENCE, else make_scene_fixtures.py's default."""
    return sys.argv[1] if __name__ == "__main__" and len(sys.argv) > 1 else os.environ.get("URT_REFERENCE", "/root/reference")


def main():
    data = mine(os.path.join(reference_root(), "Screenshots", CAPTURE))
    dst = os.path.join(HERE, "screenshot_silhouettes.json")
    text = json.dumps(data, indent=1, sort_keys=True)
    text = re.sub(r"\[\s+(\d+),\s+(\d+),\s+(\d+)\s+\]", r"[\1, \2, \3]", text)      # one span per line
    with open(dst, "w") as f:
        f.write(text + "\n")
    for name, obj in data["objects"].items():
        print(name, {e: (r["value"], r["difference"], r["spread_over_sweep"]) for e, r in obj.get("edges", {}).items()} or obj["iou_with_oracle_over_sweep"])
    for d in data["dropped_edges"]:
        print("dropped:", d["object"], d["edge"], d["value"], d["oracle"], d["spread_over_sweep"], d["reason"])
    print("->", dst)


if __name__ == "__main__":
    main()
