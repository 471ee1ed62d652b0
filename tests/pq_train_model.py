"""The numpy model of afis_pq_train (include/afis_matcher.h, "Codebook training"): one Lloyd step defined bit for bit and independent of summation order.

  assignment    the oracle's PQ encoder (oracle.pq_encode, the CPU restatement afis_pq_encode is tested against) under an oracle codebook made from the bytes of
                the current codewords
  accumulation  q(x) = rint(x * 2^30) in fp64 -> int64, summed per (sub-quantizer, code) with np.add.at, and the counts
  update        (float32)((float64) S / ((float64) count * 2^30)) where count > 0, the old bits elsewhere
and the point sampler of afis_pq_train_init_points restated on Python integers.  The sub-spaces are independent: step() runs the 16 of a 96-d set, step6() one 6-d
set on its own (what scipy's kmeans2 is given per sub-space).  Not a test module; tests/test_pq_train_host.py and tests/test_gpu_pq_train.py import it."""
import struct

import numpy as np

M_, K_, D_ = 16, 256, 6
MASK = (1 << 64) - 1


def codebook_file(codewords) -> bytes:
    """The bytes of a codebook file: 3 x int16 header and the floats (what afis_codebook_write writes)."""
    return struct.pack("<3h", M_, K_, D_) + np.ascontiguousarray(codewords, np.float32).reshape(M_, K_, D_).tobytes()


def _encode(oracle, codewords, des):
    ocb = oracle.codebook(codebook_file(codewords))
    try:
        return oracle.pq_encode(ocb, des)
    finally:
        oracle.lib.orc_codebook_free(ocb)


def assign(oracle, codewords, des):
    """labels [n][16] u8 under the codewords; equal rows are encoded once (the encoder is a function of the row)."""
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    rows, inverse = np.unique(des.view(np.dtype((np.void, 384))).ravel(), return_inverse=True)
    return _encode(oracle, codewords, np.ascontiguousarray(rows.view(np.float32).reshape(-1, 96)))[inverse.ravel()]


def assign6(oracle, cw6, x6):
    """One sub-space on its own: labels [n] of the points x6 [n][6] under cw6 [256][6].  The encoder treats its 16 sub-spaces alike and independently, so 16 points
    ride in one 96-d row against a codebook whose 16 slices are all cw6."""
    x6 = np.ascontiguousarray(x6, np.float32).reshape(-1, D_)
    n = len(x6)
    packed = np.zeros(((n + M_ - 1) // M_ * M_, D_), np.float32); packed[:n] = x6
    return _encode(oracle, np.broadcast_to(np.asarray(cw6, np.float32).reshape(1, K_, D_), (M_, K_, D_)), packed.reshape(-1, 96)).reshape(-1)[:n]


def accumulate6(x6, labels):
    """(S [256][6] int64, count [256] int64) of one sub-space's assignment."""
    q = np.rint(np.asarray(x6, np.float32).astype(np.float64) * 2.0 ** 30).astype(np.int64)
    S = np.zeros((K_, D_), np.int64); count = np.zeros(K_, np.int64)
    np.add.at(S, labels.astype(np.int64), q)
    np.add.at(count, labels.astype(np.int64), 1)
    return S, count


def update6(cw6, S, count):
    """One sub-space's codewords after the step; empty clusters keep their bits."""
    old = np.asarray(cw6, np.float32).reshape(K_, D_)
    with np.errstate(divide="ignore", invalid="ignore"):
        new = (S.astype(np.float64) / (count.astype(np.float64) * 1073741824.0)[:, None]).astype(np.float32)
    return np.where((count > 0)[:, None], new, old)


def step6(oracle, cw6, x6):
    labels = assign6(oracle, cw6, x6)
    S, count = accumulate6(x6, labels)
    return update6(cw6, S, count), labels, count


def step(oracle, codewords, des):
    """(codewords after the step, labels [n][16], count [16][256])."""
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    old = np.ascontiguousarray(codewords, np.float32).reshape(M_, K_, D_)
    labels = assign(oracle, old, des)
    new = np.empty_like(old); count = np.zeros((M_, K_), np.int64)
    for m in range(M_):
        S, count[m] = accumulate6(des[:, m * D_:(m + 1) * D_], labels[:, m])
        new[m] = update6(old[m], S, count[m])
    return new, labels, count


def train(oracle, des, init, iters, early_stop=True):
    """afis_pq_train: dict(codewords, counts, changed [iters], iters_run).  early_stop False runs every step (what the early stop must not change)."""
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    cw = np.ascontiguousarray(init, np.float32).reshape(M_, K_, D_).copy()
    counts = np.zeros((M_, K_), np.int64); changed = np.zeros(max(iters, 0), np.int64); run = 0
    prev = None
    if len(des):
        for t in range(iters):
            cw, labels, counts = step(oracle, cw, des)
            changed[t] = labels.size if prev is None else int((labels != prev).sum())
            prev = labels; run = t + 1
            if early_stop and t >= 1 and changed[t] == 0:
                break
    return {"codewords": cw, "counts": counts, "changed": changed, "iters_run": run}


def clustered(rng, n, blobs=40, sigma=0.3, spread=0.4):
    """Training points [n][96]: in every sub-space `blobs` Gaussian blobs of sigma `sigma` around centres of sigma `spread` (norms near the shipped descriptors')."""
    des = np.empty((n, 96), np.float32)
    for m in range(M_):
        centres = rng.standard_normal((blobs, D_)) * spread
        des[:, m * D_:(m + 1) * D_] = (centres[rng.integers(0, blobs, n)] + rng.standard_normal((n, D_)) * sigma).astype(np.float32)
    return des


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def init_indices(n, seed, m):
    """The 256 distinct point indices of sub-quantizer m: the first 256 steps of a Fisher-Yates shuffle driven by draw(m, j) = mix(mix(seed) + 256 m + j)."""
    a = list(range(n)) if n <= 1 << 16 else None
    moved = {}
    out = []
    for j in range(K_):
        r = j + mix((mix(seed & MASK) + K_ * m + j) & MASK) % (n - j)
        if a is not None:
            a[j], a[r] = a[r], a[j]
            out.append(a[j])
        else:
            aj, ar = moved.get(j, j), moved.get(r, r)
            moved[r], moved[j] = aj, ar
            out.append(ar)
    return out


def init_points(des, seed):
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    init = np.zeros((M_, K_, D_), np.float32)
    for m in range(M_):
        init[m] = des[init_indices(len(des), seed, m), m * D_:(m + 1) * D_]
    return init
