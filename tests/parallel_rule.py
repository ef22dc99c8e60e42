"""THE rule of include/world_class_parallel.h restated in numpy and Python floats: the joint rows along an alignment path, the speech
mask, the distortion along the path.  A helper of tests/test_parallel_rule.py and tests/test_gpu_parallel*.py, not a test module.

  pairs       pair u has a = a_lengths[u] rows of A from A_u = sum_{v<u} a_lengths[v] and b rows of B from B_u
  paths       pair u owns the slots 0 <= s < cap_u = a + b - 1; slot s is entry P_u + s, P_u = sum_{v<u} cap_v; an entry is (i, j)
  length      K' = K if 0 <= K <= cap_u else 0
  on the path s < K' and 0 <= i < a and 0 <= j < b
  live        on the path, A's mask byte of frame A_u + i not 0 and B's of frame B_u + j not 0 (None: every frame counts)
The three small functions below (slot_offsets, cell_of, both_count) are the places where a one-line mistake would sit; the tests
replace each of them by its mistake and see the GPU tests' inputs tell the difference."""
import math

import numpy as np


def slot_offsets(a_lengths, b_lengths):
    """-> (A_u, B_u, P_u, cap_u) as lists"""
    A, B, P, caps = [], [], [], []
    fa = fb = p = 0
    for a, b in zip(a_lengths, b_lengths):
        A.append(fa)
        B.append(fb)
        P.append(p)
        caps.append(a + b - 1)
        fa, fb, p = fa + a, fb + b, p + a + b - 1
    return A, B, P, caps


def cell_of(entry):
    """an entry of the path -> (i, j)"""
    return int(entry[0]), int(entry[1])


def both_count(ma, mb):
    """whether a cell counts under the two mask bytes"""
    return ma != 0 and mb != 0


def usable_length(K, cap):
    K = int(K)
    return K if 0 <= K <= cap else 0


def slot_states(a_lengths, b_lengths, path_length, path, mask_a=None, mask_b=None):
    """-> per slot: on (bool), live (bool), row_a and row_b (the packed row numbers, -1 where the slot is not on the path)"""
    A, B, P, caps = slot_offsets(a_lengths, b_lengths)
    total = sum(caps)
    path = np.asarray(path).reshape(-1, 2)
    on, live = np.zeros(total, dtype=bool), np.zeros(total, dtype=bool)
    row_a, row_b = np.full(total, -1, dtype=np.int64), np.full(total, -1, dtype=np.int64)
    for u, (a, b) in enumerate(zip(a_lengths, b_lengths)):
        Kp = usable_length(path_length[u], caps[u])
        for s in range(Kp):
            i, j = cell_of(path[P[u] + s])
            if not (0 <= i < a and 0 <= j < b):
                continue
            g = P[u] + s
            on[g], row_a[g], row_b[g] = True, A[u] + i, B[u] + j
            ma = 1 if mask_a is None else int(mask_a[A[u] + i])
            mb = 1 if mask_b is None else int(mask_b[B[u] + j])
            live[g] = both_count(ma, mb)
    return on, live, row_a, row_b


def joint_rows(a_lengths, b_lengths, rows_a, col_a, dx, rows_b, col_b, dy, path_length, path, mask_a, mask_b, joint, col_out):
    """rows_a [frames_a, ld_a], rows_b [frames_b, ld_b] (float64 or float32), joint [slots, ld_out] as it stood before the call
    -> (joint after the call, the mask bytes).  A float read is widened exactly, a float written is the (float) of the double, same
    format to same format copies the bits (numpy's casts do all three)"""
    on, live, ra, rb = slot_states(a_lengths, b_lengths, path_length, path, mask_a, mask_b)
    out = np.array(joint, copy=True)
    assert out.shape[0] == len(on)
    out[:, col_out:col_out + dx + dy] = 0.0
    out[on, col_out:col_out + dx] = rows_a[ra[on], col_a:col_a + dx].astype(out.dtype)
    out[on, col_out + dx:col_out + dx + dy] = rows_b[rb[on], col_b:col_b + dy].astype(out.dtype)
    return out, live.astype(np.uint8)


def speech_mask(lengths, column, margin, floor):
    """column: the values of the one column, packed utterance after utterance -> one byte per frame"""
    column = np.asarray(column, dtype=np.float64)
    out = np.zeros(len(column), dtype=np.uint8)
    f = 0
    for n in lengths:
        vals = [float(v) for v in column[f:f + n]]
        finite = [v for v in vals if math.isfinite(v)]
        if finite:
            least = max(finite) - float(margin)   # one rounded subtraction
            for t, v in enumerate(vals):
                out[f + t] = 1 if math.isfinite(v) and v >= least and v >= float(floor) else 0
        f += n
    return out


def cell_distances(xa, xb):
    """rows [k, dims] against rows [k, dims] -> e [k]: ascending c from 0.0, difference, product and sum rounded apart, the root
    correctly rounded -- the local cost of align_rule.local_costs on the cells of a path"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    acc = np.zeros(xa.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(xa.shape[1]):
            d = xa[:, c] - xb[:, c]
            acc = acc + d * d
        return np.sqrt(acc)


def path_distortion(a_lengths, b_lengths, rows_a, col_a, rows_b, col_b, dims, path_length, path, mask_a=None, mask_b=None):
    """-> (sum [pairs] float64, count [pairs] int64, cell [slots] float64)"""
    on, live, ra, rb = slot_states(a_lengths, b_lengths, path_length, path, mask_a, mask_b)
    _, _, P, caps = slot_offsets(a_lengths, b_lengths)
    cell = np.zeros(len(on))
    cell[on] = cell_distances(np.asarray(rows_a)[ra[on], col_a:col_a + dims], np.asarray(rows_b)[rb[on], col_b:col_b + dims])
    sums, counts = np.zeros(len(caps)), np.zeros(len(caps), dtype=np.int64)
    for u, cap in enumerate(caps):
        total, k = 0.0, 0
        for s in range(cap):
            if live[P[u] + s]:
                e = float(cell[P[u] + s])
                total = e if k == 0 else total + e   # strictly sequential, starting at the first term
                k += 1
        sums[u], counts[u] = total, k
    return sums, counts, cell


def mcd_db(total, count):
    """mel-cepstral distortion in dB of a sum of distances over count cells"""
    return (10.0 / math.log(10.0)) * math.sqrt(2.0) * total / count


DB_IN_C0 = math.log(10.0) / 10.0   # one decibel of frame power in units of c0 (the header derives it from the codec)
