"""What a slab window `d` (fields.slab_window) holds of a whole-grid numpy array, and the planes next to it.  Shared by
tests/projection_slab_worker.py (one window per rank) and tests/test_fields_windows.py (every window in one process)."""
import numpy as np


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cell(a, d):
    return a[d.c0:d.c1]


def zface(a, d):
    return a[d.c0:d.c1 + 1]


def faces(arrs, d):
    return [cell(arrs[0], d), cell(arrs[1], d), zface(arrs[2], d)]


def halo(a, d):
    """the planes next to the window, as an exchange would deliver them; None where the grid ends"""
    return (dev(a[d.c0 - 1]) if d.c0 > 0 else None, dev(a[d.c1]) if d.c1 < d.gz else None)
