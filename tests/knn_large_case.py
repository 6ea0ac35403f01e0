"""Clouds of the large-k outlier-filter tests (k = mean_k + 1 beyond the per-lane lists of the normals kernels) and their
oracle results, computed once per process and shared by the tests that need them."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def room_cloud():
    """30 000 floor points, 10 000 wall points and 800 uniform outliers, shuffled (the cloud of
    test_gpu_normals.py::test_local_outlier_removal_matches_oracle at half the size, seed 31)."""
    rng = np.random.RandomState(31)
    plane = np.stack([rng.uniform(-2, 2, 30000), rng.uniform(-2, 2, 30000), 0.003 * rng.normal(size=30000)], 1)
    wall = np.stack([np.full(10000, 2.0), rng.uniform(-2, 2, 10000), rng.uniform(0, 1.5, 10000)], 1)
    pts = np.concatenate([plane, wall, rng.uniform(-2, 2, (800, 3))]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def lattice_cloud():
    """24 x 24 x 12 lattice at 0.05 spacing, shuffled: hundreds of candidates tie at the k-th distance."""
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    pts = g.astype(np.float32) * np.float32(0.05)
    pts = pts[np.random.RandomState(5).permutation(len(pts))]
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def room_with_far_cluster():
    """The room plus 50 points 30 m away: their neighbours lie mostly in the room, so they are resolved only by the block that
    covers the whole cloud."""
    rng = np.random.RandomState(32)
    cluster = (np.array([30.0, 0.5, 0.2]) + 0.05 * rng.normal(size=(50, 3))).astype(np.float32)
    pts = np.concatenate([room_cloud(), cluster])
    pts = pts[rng.permutation(len(pts))]
    pts.setflags(write=False)
    return pts


_CLOUDS = {"room": room_cloud, "lattice": lattice_cloud, "far": room_with_far_cluster}
_ORACLE = {}


def cloud(name, first=None, twice=False):
    pts = _CLOUDS[name]()
    if first is not None:
        pts = pts[:first]
    if twice:
        pts = np.concatenate([pts, pts])
    return pts


def oracle(ob, name, mean_k, factor, first=None, twice=False):
    """(inlier mask, first-pass mean distances) of the CPU oracle on cloud(name, first, twice); cached, read-only."""
    key = (name, mean_k, factor, first, twice)
    if key not in _ORACLE:
        inl, md = ob.local_outlier_removal(cloud(name, first, twice), mean_k, factor)
        inl.setflags(write=False); md.setflags(write=False)
        _ORACLE[key] = (inl, md)
    return _ORACLE[key]
