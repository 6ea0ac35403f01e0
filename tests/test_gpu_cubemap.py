"""CubeMapRenderer on the GPU (e3d_render_cube_map, bin/CubeMapRenderer) against the numpy restatement of tests/cubemap_ref.py:
colour, depth (as bits) and sweep counts equal, no pixel left out; and the chain CubeMapRenderer -> SfMScaleEstimator."""
import os
import signal
import subprocess
import time

import numpy as np
import pytest

import cubemap_ref as cr
import sfm_case
from cli_util import BIN, write_ply_xyz
from test_cubemap_host import check_scale_estimator_outputs, run_scale_estimator, tie_cloud

pytestmark = pytest.mark.gpu

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_equal(got, want, what=""):
    assert got[0].dtype == np.uint8 and got[1].dtype == F
    assert np.array_equal(got[0], want[0]), (what, "colour", np.argwhere((got[0] != want[0]).any(-1))[:5])
    assert np.array_equal(_u32(got[1]), _u32(want[1])), (what, "depth", np.argwhere(_u32(got[1]) != _u32(want[1]))[:5])
    assert np.array_equal(got[2], want[2]), (what, "sweeps", got[2], want[2])


@pytest.mark.parametrize("size,n", [(3, 40), (4, 100), (17, 900), (17, 30), (256, 60000), (256, 400000)])
@pytest.mark.parametrize("fill", [False, True])
def test_random_clouds_with_ties_bit_exact(e3d, size, n, fill):
    xyz, rgb = tie_cloud(100 + size + n, n)                              # quantised coordinates, non-finite points mixed in
    assert not np.isfinite(xyz).all()
    want = cr.render(xyz, rgb, size, fill)
    got = e3d.render_cube_map(xyz, rgb, size, fill)
    _assert_equal(got, want, (size, n, fill))
    if fill and size == 256 and n == 60000:
        assert want[2].max() >= 3


@pytest.mark.parametrize("fill", [False, True])
def test_no_points(e3d, fill):
    c, d, s = e3d.render_cube_map(np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), 16, fill)
    assert c.shape == (6, 16, 16, 3) and (c == 0).all() and np.isinf(d).all() and (d > 0).all() and (s == 0).all()
    _assert_equal((c, d, s), cr.render(np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), 16, fill))


def test_argument_errors(e3d):
    xyz, rgb = tie_cloud(1, 50, False)
    with pytest.raises(e3d.E3DError, match="size"):
        e3d.render_cube_map(xyz, rgb, 2)


def room_with_blind_cone(synth, n=6_000_000, cone_deg=40.0):
    """the synthetic room seen from 0.5 m in front of the wall x = 0, turned so that the floor lies along +Y (the down face);
    colours are a function of position; the points inside a cone below the scanner are dropped"""
    xyz, _, _ = synth.make_scan(n, (0.5, 5.0, 1.5), 0.0, seed=11)
    p = xyz.numpy()
    p = np.stack([p[:, 0], -p[:, 2], p[:, 1]], 1).astype(F)              # room z (up) -> -y
    cosang = p[:, 1] / np.linalg.norm(p, axis=1)
    p = np.ascontiguousarray(p[cosang < np.cos(np.deg2rad(cone_deg))])
    rgb = np.stack([(p[:, 0] * 37) % 256, (p[:, 1] * 53 + 90) % 256, (p[:, 2] * 29 + 180) % 256], 1).astype(np.uint8)
    return p, rgb


def test_synthetic_room_with_blind_cone(e3d, synth):
    xyz, rgb = room_with_blind_cone(synth)
    # size 96: the cone (40 degrees, so that it stays out of the side faces) is a disc of radius 48 tan 40 = 40 pixels, i.e. 28
    # sweeps (Chebyshev distance from its centre); the wall patch the left face sees gets 2.7 points per pixel
    want = cr.render(xyz, rgb, 96)
    got = e3d.render_cube_map(xyz, rgb, 96)
    print("sweeps", want[2])
    _assert_equal(got, want)
    assert want[2][cr.FACES.index("down")] >= 20                         # more than one look at the sweeps' words is needed
    assert (want[2] == 0).any()                                          # the wall half a metre away fills its face
    _assert_equal(e3d.render_cube_map(xyz, rgb, 96, fill=False), cr.render(xyz, rgb, 96, fill=False))


def test_two_calls_identical_bytes(e3d, synth):
    xyz, rgb = tie_cloud(77, 500000)
    a = e3d.render_cube_map(xyz, rgb, 128)
    b = e3d.render_cube_map(xyz, rgb, 128)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)


def _read_ppm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = (int(v) for v in head[1].split())
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_cli_files_equal_restatement(e3d, tmp_path):
    xyz, rgb = sfm_case.room_scan(3, 30000)
    xyz[::1000, 0] = np.nan
    write_ply_xyz(str(tmp_path / "scan.ply"), xyz, rgb)
    base = str(tmp_path / "out") + ".scan.ply"
    r = _run([os.path.join(BIN, "CubeMapRenderer"), "-c", str(tmp_path / "scan.ply"), "-o", base, "--size", "96"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("Finished!")
    want_c, want_d, _ = cr.render(xyz, rgb, 96)
    assert open(base + ".intrinsics.txt", "rb").read() == cr.intrinsics_text(96).encode()
    for i, name in enumerate(cr.FACES):
        assert open(base + "." + name + ".depth", "rb").read() == np.ascontiguousarray(want_d[i], "<f4").tobytes(), name
        ppm = str(tmp_path / (name + ".ppm"))
        subprocess.check_call([os.path.join(BIN, "e3d_imread_gray"), "--color", base + "." + name + ".png", ppm])      # the project's own PNG reader
        assert np.array_equal(_read_ppm(ppm), want_c[i]), name


def test_tools_chained_recover_the_scale(e3d, tmp_path):
    case = sfm_case.build(str(tmp_path), k=3.7, with_scan3=False, write_depth=False)
    for name in ("scan1.ply", "scan2.ply"):
        r = _run([os.path.join(BIN, "CubeMapRenderer"), "-c", os.path.join(case["scans"], name), "-o", os.path.join(case["images"], name),
                  "--size", str(sfm_case.SIZE)])
        assert r.returncode == 0, r.stdout + r.stderr
    r = run_scale_estimator(case)
    assert r.returncode == 0, r.stdout + r.stderr
    check_scale_estimator_outputs(case, r)


class _Limit:
    """a time limit for one step of a test (SIGALRM)"""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def fire(signum, frame):
            raise TimeoutError("%s took longer than %d s" % (self.what, self.seconds))
        self.old = signal.signal(signal.SIGALRM, fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)
        return False


def closed_room_cloud(n, cone_deg, seed=21):
    """n directions, uniform on the sphere except a blind cone around +Y (below the scanner), on the walls of a box"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3), dtype=F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[d[:, 1] < np.cos(np.deg2rad(cone_deg))]
    lo, hi = np.array([-4.0, -1.2, -3.0], F), np.array([2.5, 1.6, 5.0], F)
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    xyz = np.ascontiguousarray((d * t[:, None]).astype(F))
    rgb = np.stack([(xyz[:, 0] * 61) % 256, (xyz[:, 1] * 97 + 50) % 256, (xyz[:, 2] * 43 + 120) % 256], 1).astype(np.uint8)
    return xyz, rgb


def test_at_size_20m_points_2048(e3d):
    xyz, rgb = closed_room_cloud(21_000_000, 25.0)
    assert len(xyz) >= 19_500_000
    t0 = time.time()
    with _Limit(300, "e3d_render_cube_map"):
        got = e3d.render_cube_map(xyz, rgb, 2048)
    t1 = time.time()
    with _Limit(900, "the numpy restatement"):
        want = cr.render(xyz, rgb, 2048)
    print("points %d sweeps %s; call %.2f s, restatement %.1f s" % (len(xyz), want[2], t1 - t0, time.time() - t1))
    _assert_equal(got, want)
    assert want[2][cr.FACES.index("down")] >= 300
