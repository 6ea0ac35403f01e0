"""PointCloudCleaner with the parameters the reference documents for the ETH3D point clouds, `--filter 270,1.15 --filter 20,1.15`:
the first pass needs the 271 nearest neighbours of every point."""
import os
import subprocess

import numpy as np
import pytest

import knn_large_case as case
from cli_util import BIN, write_ply_xyz

pytestmark = pytest.mark.gpu


def test_point_cloud_cleaner_eth3d_filters(tmp_path, ob):
    pts = case.cloud("room")
    rgb = np.random.RandomState(33).randint(0, 256, (len(pts), 3)).astype(np.uint8)
    assert len(pts) == 40800
    path = str(tmp_path / "scan.ply")
    write_ply_xyz(path, pts, rgb=rgb)
    r = subprocess.run([os.path.join(BIN, "PointCloudCleaner"), "--in", path, "--filter", "270,1.15", "--filter", "20,1.15"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Applying filter with knn = 270, factor = 1.15 ..." in r.stderr and "Applying filter with knn = 20, factor = 1.15 ..." in r.stderr

    def read(p):
        raw = open(p, "rb").read()
        h = raw.index(b"end_header\n") + 11
        header = raw[:h].decode()
        n = int(header.split("element vertex ")[1].split()[0])
        rec = np.frombuffer(raw, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), n, h)
        assert len(raw) - h - 15 * n == 4 * 12 + 4 * 5 + 4 * 2 + 4 * 2 and "property uchar red" in header and "element camera 1" in header
        return rec
    inl, outl = read(path + ".inliers.ply"), read(path + ".outliers.ply")
    k1, _ = case.oracle(ob, "room", 270, 1.15)
    p1, c1 = pts[k1], rgb[k1]
    k2, _ = ob.local_outlier_removal(p1, 20, 1.15)
    assert np.array_equal(inl["p"], p1[k2]) and np.array_equal(inl["c"], c1[k2])
    # the removed points in removal order: the first pass's, then the second's
    exp_out_p = np.concatenate([pts[~k1], p1[~k2]]); exp_out_c = np.concatenate([rgb[~k1], c1[~k2]])
    assert np.array_equal(outl["p"], exp_out_p) and np.array_equal(outl["c"], exp_out_c)
    assert len(inl) + len(outl) == len(pts) and 0 < len(outl) < len(pts) // 4
