"""HIP-event times of the PointCloudEdit kernels on one MI355X.

    python tools/bench_edit.py [--points 50000000] [--reps 7]

Per operation: median (min - max) of the kernel time the library reports (e3d_edit_kernel_ms) over --reps calls after two warm-up
calls, next to the bytes the operation has to move and the bandwidth that gives."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
e3d = importlib.import_module("dataset-pipeline_amd")


def timed(E, call, reps):
    ms = []
    for i in range(reps + 2):
        call()
        if i >= 2:
            ms.append(E.kernel_ms())
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, W, H = a.points, 1280, 960
    rng = np.random.default_rng(0)
    z = rng.uniform(0.5, 60.0, n).astype(np.float32)
    xyz = np.stack([rng.uniform(-0.8, 0.8, n).astype(np.float32) * z, rng.uniform(-0.6, 0.6, n).astype(np.float32) * z, z], 1)
    del z
    view = e3d.edit_view(W, H, None, 0.1, 100.0)
    E = e3d.PointCloudEdit(xyz)

    def polygon(m):
        t = np.linspace(0, 2 * np.pi, m, endpoint=False)
        r = 1 + 0.3 * np.cos(5 * t)
        return np.stack([W / 2 + 0.35 * W * r * np.cos(t), H / 2 + 0.35 * H * r * np.sin(t)], 1)

    rows = []

    def row(name, bytes_per_point, t, note=""):
        med, lo, hi = t
        gb = bytes_per_point * n / 1e9
        rows.append("%-34s %8.3f ms (%.3f - %.3f)  %5.1f B/point = %6.3f GB -> %6.2f TB/s  %s" % (name, med, lo, hi, bytes_per_point, gb, gb / med, note))

    for m in (8, 40, 400):
        P = polygon(m)
        t = timed(E, lambda: E.lasso(view, P, "replace"), a.reps)
        row("lasso replace, %d vertices" % m, 13, t, "selected %d" % E.selection_count())
    P = polygon(40)
    row("lasso add, 40 vertices", 14, timed(E, lambda: E.lasso(view, P + 100, "add"), a.reps), "selected %d" % E.selection_count())
    depth = np.full((H, W), np.inf, np.float32)
    depth[:, : W // 2] = 20.0
    row("lasso replace, 40 vertices, depth", 13, timed(E, lambda: E.lasso(view, P, "replace", depth), a.reps), "selected %d (+ 4 B gathered per inside point)" % E.selection_count())
    pts = np.array([[0, 0, 30], [1, 0, 30.5], [0, 1, 29.5]], np.float32)
    row("beyond_plane", 13, timed(E, lambda: E.beyond_plane(view, pts, [0, 0, 0], False), a.reps), "selected %d" % E.selection_count())
    row("beyond_plane, visible only", 13, timed(E, lambda: E.beyond_plane(view, pts, [0, 0, 0], True), a.reps), "selected %d" % E.selection_count())
    clicks = np.stack([np.linspace(100, 1100, 8), np.linspace(100, 800, 8)], 1)
    row("pick, 1 click", 12, timed(E, lambda: E.pick(view, clicks[:1]), a.reps))
    row("pick, 8 clicks", 12, timed(E, lambda: E.pick(view, clicks), a.reps))
    # compaction: counts (1 B) + copy (1 B flag, 12 B read and 12 B written per kept point)
    for name, flags in (("10 % selected", rng.random(n) < 0.1), ("50 % selected", rng.random(n) < 0.5)):
        k = E.set_selection(flags)
        out = np.zeros((k, 3), np.float32)
        lib = e3d.lib()

        def extract():
            import ctypes
            assert lib.e3d_edit_extract_selected(E._h, ctypes.c_void_p(out.ctypes.data), k) == k
        row("extract_selected, " + name, 2 + 24.0 * k / n, timed(E, extract, max(a.reps // 2, 1)), "kernels only; the copy to the host is not in it")
    E.delete_selected()
    row("delete_selected, 50 % selected", 2 + 24.0 * len(E) / n, (E.kernel_ms(),) * 3, "one call")
    print("PointCloudEdit kernels, %d points, view %d x %d" % (n, W, H))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
