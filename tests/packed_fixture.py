"""How tests/golden/heads_train.npz stores its arrays, for tools/make_golden_heads_train.py (which packs) and
tests/heads_train_ref.load_golden (which unpacks): integers as zigzag byte planes, reference results as integers of step
max|v| * 2^-QBITS per array (the rounding is at most 2^-(QBITS + 1) = 1.2e-7 of the array's maximum), the upstream gradients of
{-1, -1/2, 0, 1/2, 1} three to a byte.  Plain fp32 arrays of the same data deflate to 1.1 MB, above what a committed file may hold.
"""
import numpy as np
import torch

QBITS = 22


def planes_of(q, width):
    """integers -> their zigzag codes (0, -1, 1, -2, .. -> 0, 1, 2, 3, ..) as `width` byte planes [width,n]: the planes deflate far
    better than the words."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    u = np.where(q < 0, -2 * q - 1, 2 * q).astype('<u8')
    assert int(u.max()) < 1 << (8 * width)
    return np.ascontiguousarray(u.view(np.uint8).reshape(-1, 8)[:, :width].T)


def ints_of(planes):
    width, n = planes.shape
    b = np.zeros((n, 8), dtype=np.uint8)
    b[:, :width] = planes.T
    u = b.view('<u8').reshape(-1).astype(np.int64)
    return np.where(u & 1, -(u + 1) // 2, u // 2)


def pack5(v):
    """values of {-1, -1/2, 0, 1/2, 1} -> one byte per three of them (base 5)."""
    d = np.rint(np.asarray(v, dtype=np.float64).reshape(-1) * 2 + 2).astype(np.int64)
    assert d.min() >= 0 and d.max() <= 4
    d = np.concatenate([d, np.zeros(-d.size % 3, dtype=np.int64)]).reshape(-1, 3)
    return (d[:, 0] * 25 + d[:, 1] * 5 + d[:, 2]).astype(np.uint8)


def unpack5(codes, shape):
    c = codes.astype(np.int64)
    d = np.stack([c // 25, c // 5 % 5, c % 5], 1).reshape(-1)[:int(np.prod(shape))]
    return torch.from_numpy(((d - 2) / 2).astype(np.float32).reshape(shape))


def pack(v):
    """fp32 array -> (integers of step max|v| * 2^-QBITS as three byte planes, step)."""
    v = np.asarray(v, dtype=np.float64)
    step = float(np.abs(v).max()) * 2.0 ** -QBITS or 1.0
    return planes_of(np.rint(v / step), 3), step


def unpack(planes, step, shape):
    return torch.from_numpy(ints_of(planes).astype(np.float64).reshape(shape) * step)
