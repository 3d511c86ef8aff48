"""The storage order restated in numpy (sas_api.cpp: storage_order, hilbert3; DESIGN.md 3, "Storage order"): slot -> caller's index,
ordered by (group id, Hilbert index of the mean at 10 bits per axis, caller's index).

Every float operation is one correctly rounded float32 operation, in the library's order: the bounds are float32 min / max over the finite
entries, inv = 1023 / (hi - lo) where hi > lo and 0 elsewhere, u = (v - lo) * inv clamped to [0, 1023] (a non-finite v: 0), and the
conversion truncates.  ``storage_order`` is vectorised (Skilling's transform on whole arrays, a stable argsort of group << 32 | index);
``storage_order_loop`` is the same thing element by element with Python integers and ``sorted``, for tests/test_order_cpu.py."""
import numpy as np

BITS = 10
QMAX = np.float32((1 << BITS) - 1)


def hilbert3(x, y, z, bits=BITS):
    """3-D Hilbert index of Python integers (Skilling's transpose form), as sas_api.cpp writes it."""
    X = [int(x), int(y), int(z)]
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:
        P = Q - 1
        for i in range(3):
            if X[i] & Q:
                X[0] ^= P
            else:
                t = (X[0] ^ X[i]) & P
                X[0] ^= t
                X[i] ^= t
        Q >>= 1
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = 0
    Q = M
    while Q > 1:
        if X[2] & Q:
            t ^= Q - 1
        Q >>= 1
    X = [v ^ t for v in X]
    code = 0
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            code = (code << 1) | ((X[i] >> b) & 1)
    return code


def hilbert3_np(q, bits=BITS):
    """The same for ``q [n,3]`` of unsigned integers below 2**bits: uint64 ``[n]``."""
    X = [np.asarray(q[:, k], np.uint32).copy() for k in range(3)]
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            on = (X[i] & np.uint32(Q)) != 0
            t = np.where(on, np.uint32(0), (X[0] ^ X[i]) & P)
            X[0] = np.where(on, X[0] ^ P, X[0] ^ t)   # (i == 0 and off: t is 0, nothing changes)
            X[i] = np.where(on, X[i], X[i] ^ t) if i else X[0]
        Q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & np.uint32(Q)) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    X = [v ^ t for v in X]
    code = np.zeros(X[0].shape, np.uint64)
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            code = (code << np.uint64(1)) | ((X[i] >> np.uint32(b)) & np.uint32(1)).astype(np.uint64)
    return code


def bounds(means):
    """(lo, hi, inv), float32 ``[3]`` each, over the finite coordinates of ``means [n,3]``."""
    m = np.asarray(means, np.float32).reshape(-1, 3)
    fin = np.isfinite(m)
    lo = np.where(fin, m, np.float32(np.inf)).min(axis=0, initial=np.float32(np.inf)).astype(np.float32)
    hi = np.where(fin, m, np.float32(-np.inf)).max(axis=0, initial=np.float32(-np.inf)).astype(np.float32)
    inv = np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            if hi[k] > lo[k]:
                inv[k] = QMAX / (hi[k] - lo[k])
    return lo, hi, inv


def quantise(means):
    """uint32 ``[n,3]``: the cell of every coordinate in the 1024-cell grid over the finite coordinates' box."""
    m = np.asarray(means, np.float32).reshape(-1, 3)
    lo, hi, inv = bounds(m)
    with np.errstate(all="ignore"):
        u = np.where(np.isfinite(m), (m - lo[None, :]) * inv[None, :], np.float32(0.0)).astype(np.float32)
    u = np.where(u > 0, np.minimum(u, QMAX), np.float32(0.0)).astype(np.float32)   # (a NaN product becomes 0)
    return u.astype(np.uint32)   # truncates


def keys(means, group_id=None):
    """uint64 ``[n]``: group << 32 | Hilbert index."""
    h = hilbert3_np(quantise(means))
    if group_id is None:
        return h
    return (np.asarray(group_id, np.uint8).astype(np.uint64) << np.uint64(32)) | h


def storage_order(means, group_id=None):
    """int32 ``[n]``: slot -> caller's index."""
    return np.argsort(keys(means, group_id), kind="stable").astype(np.int32)


def storage_order_loop(means, group_id=None):
    """The same, one element at a time: float32 scalars, Python integers, ``sorted`` on (key, index)."""
    m = np.asarray(means, np.float32).reshape(-1, 3)
    n = m.shape[0]
    lo, hi = [np.float32(np.inf)] * 3, [np.float32(-np.inf)] * 3
    for i in range(n):
        for k in range(3):
            v = m[i, k]
            if np.isfinite(v):
                lo[k], hi[k] = min(lo[k], v), max(hi[k], v)
    with np.errstate(all="ignore"):
        inv = [QMAX / (hi[k] - lo[k]) if hi[k] > lo[k] else np.float32(0.0) for k in range(3)]
        key = []
        for i in range(n):
            q = []
            for k in range(3):
                v = m[i, k]
                u = (v - lo[k]) * inv[k] if np.isfinite(v) else np.float32(0.0)
                u = min(max(u, np.float32(0.0)), QMAX)
                q.append(int(u))
            g = int(group_id[i]) if group_id is not None else 0
            key.append((g << 32) | hilbert3(*q))
    return np.asarray(sorted(range(n), key=lambda i: (key[i], i)), np.int32)
