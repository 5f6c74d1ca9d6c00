"""What tests/test_gpu_admm.py, test_gpu_admm_lin.py, test_gpu_admm_soc.py and test_gpu_admm_refusals.py share: moving arrays to and
from the device, comparing them bit for bit, and the host's rule for the knots the row update stages at a time."""
import numpy as np
import torch


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached references are read-only)


def bits(t):
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def np_same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def np_same_or_nan(a, b):
    """The same bits, except that a NaN need only meet a NaN: the sign and payload of a NaN that an operation makes (Inf - Inf) are
    the platform's, and the host's differ from the device's."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np_same(np.where(na, 0, a).astype(a.dtype), np.where(nb, 0, b).astype(b.dtype))


def host(t, batch):
    return t.cpu().numpy().reshape(batch, -1)


def knot_chunk(nx, nu, mx, mu):
    """The knots the update kernel stages at a time (admm_rows_knot_chunk in csrc/admm_rows.hip): what fits 4096 elements, 1 .. 64."""
    per = mx * nx + mu * nu + nx + nu + 2 * (mx + mu)
    return max(1, min(64, 4096 // per))
