"""Float64 arbiters and per-element bars for the device-built second-order and degree operators (csrc/spgemm.hip,
pygsd_segment_sum_f32, pygsd_degree_scale_f32).  Plain numpy / scipy: imported by the CPU tests that hold the arbiters to
the reference's fixtures and by tests/test_gpu_operator_fuzz.py.

Every arbiter returns a `Ref`: the positions where at least one term lands (row-major), the float64 value there, the bar
`bound` a present element must meet, and `cancel`, the magnitude at or below which an element may be present or absent
(its sum can cancel to zero on one side and not the other).  `exact` arbiters hold presence bit-exactly.

Rounding units: u = 2^-24 (float32), 2^-52 = 2 x float64's unit roundoff.  A float64 sum of m terms, each a product
rounded at most twice, is within gamma_{m+1} sum|t| ~ (m + 1) 2^-53 sum|t| of the exact value; the device and the arbiter
each carry that error, so they are within (m + 1) 2^-52 sum|t| of each other, and one float32 rounding of the device's
sum adds u |value| (and u times that error, absorbed by writing m + 2).  Hence CANCEL(m) = (m + 2) 2^-52 sum|t|.

float32 sums on the device (pygsd_segment_sum_f32): rows of at most PYGSD_LONG_ROW = 4096 entries are summed by a
16-lane team, each lane sequentially over ceil(n / 16) entries, then 4 butterfly levels: a tree of height
min(n - 1, ceil(n / 16) + 3), so the error is at most gamma_h sum|w| (Higham, Accuracy and Stability, 4.2).  Longer rows
take the segment-parallel path (hub_dot_kernel, hub_finish_kernel): segments of 4096 entries, 256 threads each summing
16 of them sequentially, a 64-lane butterfly (6 levels) and the 4 wavefronts' pairwise sum (2 levels), then the
ceil(n / 4096) segment partials summed sequentially: height 16 + 6 + 2 + ceil(n / 4096)."""
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24
E52 = 2.0 ** -52
U64 = 2.0 ** -53
LONG_ROW = 4096
POWF_ULP = 2            # powf(d, -0.5f): the HIP math library's documented bound for powf is 2 ulp (1 ulp <= 2u)
SECOND_ORDER = 1 + 2.0 ** -10   # products of two first-order terms, each <= 2^-10 here, are absorbed by this factor


class Ref(NamedTuple):
    n_cols: int
    row: np.ndarray
    col: np.ndarray
    val: np.ndarray
    bound: np.ndarray
    cancel: np.ndarray
    exact: bool


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1 - k * U)


def team_height(n):
    """Height of pygsd_segment_sum_f32's summation tree over a row of n entries."""
    n = np.asarray(n, dtype=np.int64)
    team = np.minimum(np.maximum(n - 1, 0), -(-n // 16) + 3)
    return np.where(n <= LONG_ROW, team, 24 + -(-n // LONG_ROW))


def csr(r, c, v, shape):
    m = sp.coo_matrix((np.asarray(v, dtype=np.float64), (np.asarray(r), np.asarray(c))), shape=shape).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def at(m, row, col):
    """Values of the (canonical) CSR m at the positions (row, col), 0 where m holds no entry."""
    m = m.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    coo = m.tocoo()
    width = max(m.shape[1], 1)
    keys = coo.row.astype(np.int64) * width + coo.col
    want = np.asarray(row, dtype=np.int64) * width + np.asarray(col, dtype=np.int64)
    pos = np.minimum(np.searchsorted(keys, want), max(keys.size - 1, 0))
    hit = keys.size > 0
    out = np.zeros(want.size)
    if hit:
        ok = keys[pos] == want
        out[ok] = coo.data[pos[ok]]
    return out


def pattern(m):
    m = m.tocsr()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    coo = m.tocoo()
    return coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data


# ---------------------------------------------------------------------------------------------------------------- gram
def gram_terms(r, c, w, n_rows, n_cols, scale=None, scale_err=None):
    """C = B^T diag(s) B of B = COO (r, c, w) [n_rows, n_cols] (duplicates add): (pattern row, col, float64 value,
    sum|t|, m = number of products, sum|t| delta_k for a relative error delta_k of scale k) at every position where a
    product lands."""
    w = np.asarray(w, dtype=np.float64)
    s = np.ones(n_rows) if scale is None else np.asarray(scale, dtype=np.float64)
    b = csr(r, c, w, (n_rows, n_cols))
    ab = csr(r, c, np.abs(w), (n_rows, n_cols))
    cnt = csr(r, c, np.ones(w.size), (n_rows, n_cols))
    mag = ab.T @ sp.diags(np.abs(s)) @ ab
    row, col, sum_abs = pattern(mag)
    val = at(b.T @ sp.diags(s) @ b, row, col)
    m = at(cnt.T @ cnt, row, col)
    pert = np.zeros(row.size) if scale_err is None else at(ab.T @ sp.diags(np.abs(s) * scale_err) @ ab, row, col)
    return row, col, val, sum_abs, m, pert


def gram_ref(r, c, w, n_rows, n_cols, scale=None, exact=False):
    """Bar of sparse_gram.gram: one float32 rounding of a float64 sum, |got - C| <= u |C| + (m + 2) 2^-52 sum|t|.
    exact: integer weights and a power-of-two (or absent) scale, whose float64 sums are exact on both sides."""
    row, col, val, sum_abs, m, _ = gram_terms(r, c, w, n_rows, n_cols, scale)
    cancel = np.zeros(row.size) if exact else (m + 2) * E52 * sum_abs
    return Ref(n_cols, row, col, val, U * np.abs(val) + cancel, cancel, exact)


# ----------------------------------------------------------------------------------------------------------- intersect
def intersect_ref(a, b):
    """sparse_gram.intersect on two canonical scipy CSRs: a column present in both rows with a + b != 0 (in float64)
    keeps float32((a + b) * 0.5).  Returns (index [2, nnz], float32 values): the arithmetic is exact, held bit-exact."""
    a, b = a.tocsr(), b.tocsr()
    rows, cols, vals = [], [], []
    for i in range(a.shape[0]):
        ca, va = a.indices[a.indptr[i]:a.indptr[i + 1]], a.data[a.indptr[i]:a.indptr[i + 1]]
        cb, vb = b.indices[b.indptr[i]:b.indptr[i + 1]], b.data[b.indptr[i]:b.indptr[i + 1]]
        both, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
        ia, ib = ia[np.argsort(both)], ib[np.argsort(both)]
        s = va[ia].astype(np.float32).astype(np.float64) + vb[ib].astype(np.float32).astype(np.float64)
        keep = s != 0
        rows.append(np.full(int(keep.sum()), i))
        cols.append(np.sort(both)[keep])
        vals.append((s[keep] * 0.5).astype(np.float32))
    if not rows:
        return np.zeros((2, 0), np.int64), np.zeros(0, np.float32)
    return np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64), np.concatenate(vals)


# ------------------------------------------------------------------------------------------------------------ features
def ill_conditioned_sums(ei, size, w):
    """Real-valued signed weights whose row or column sum is within 1e-6 of zero relative to its sum|w|: a float32 sum
    there has no relative accuracy to hold.  Such draws are skipped and counted, not loosened."""
    if w is None:
        return False
    w = np.asarray(w, dtype=np.float64)
    if np.all(w == np.round(w)):
        return False                                   # integer sums are exact in float32 and in float64
    for axis in (0, 1):
        s = np.bincount(ei[axis], weights=w, minlength=size)
        a = np.bincount(ei[axis], weights=np.abs(w), minlength=size)
        if np.any((a > 0) & (np.abs(s) <= 1e-6 * a)):
            return True
    return False


def features_refs(ei, size, w=None):
    """(A_in, A_out) of directed_features_in_out: A_in = A^T diag(1/c) A, A_out = A diag(1/r) A^T with c, r the column
    and row sums (0 -> 1).  On the device c and r are float32 team sums: a relative error delta_k <= gamma_h(len_k)
    sum|w|_k / |c_k| of the scale (1/c_k rounded in float64 adds 2^-53), so each term t_k may be off by |t_k| delta_k.
    Bar: u |C| + (m + 2) 2^-52 sum|t| + sum |t_k| delta_k (both the gram bar and the scale's), times SECOND_ORDER."""
    ei = np.asarray(ei, dtype=np.int64)
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    exact_sums = bool(np.all(w == np.round(w)))
    out = []
    for k_axis, other in ((0, 1), (1, 0)):       # A_in: B = A, scale 1/c; A_out: B = A^T, scale 1/r
        k_ids = ei[k_axis]
        s = np.bincount(ei[other], weights=w, minlength=size)   # node k's scale: column sum (A_in), row sum (A_out)
        a = np.bincount(ei[other], weights=np.abs(w), minlength=size)
        n = np.bincount(ei[other], minlength=size)
        zero = s == 0
        kappa = a / np.where(zero, 1.0, np.abs(s))     # the arbiter's own float64 sum adds (n + 1) 2^-53 kappa
        rel = np.where(zero, 0.0, (gamma(0 if exact_sums else team_height(n)) + (n + 1) * U64) * kappa)
        s[zero] = 1
        row, col, val, sum_abs, m, pert = gram_terms(k_ids, ei[other], w, size, size, 1.0 / s, rel + U64)
        cancel = ((m + 2) * E52 * sum_abs + pert) * SECOND_ORDER
        out.append(Ref(size, row, col, val, U * np.abs(val) + cancel, cancel, False))
    return out


# -------------------------------------------------------------------------------------------------------------- degree
def degree_ref(ei, n, w=None, signed=False):
    """in_out_degree's columns in float64 and the per-element bar.  Unit or integer weights: bit-exact (float32 sums of
    integers below 2^24 are exact).  Real weights: the float32 team sums' gamma_h sum|w| over the row; signed ones first
    coalesce duplicates with another team sum (heights add), and max(a, 0) is 1-Lipschitz so the split into positive and
    negative parts adds nothing.  Returns (float64 [n, 2 or 4], bound of the same shape)."""
    ei = np.asarray(ei, dtype=np.int64)
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    exact = bool(np.all(w == np.round(w))) and np.abs(w).sum() < 2 ** 24
    if not signed:
        aw = np.abs(w)
        cols, bounds = [], []
        for axis in (0, 1):
            s = np.bincount(ei[axis], weights=aw, minlength=n)
            cnt = np.bincount(ei[axis], minlength=n)
            cols.append(s)
            bounds.append(np.zeros(n) if exact else gamma(team_height(cnt)) * s + cnt * E52 * s)
        return np.stack(cols, 1), np.stack(bounds, 1)
    a = csr(ei[0], ei[1], w, (n, n))
    dup = csr(ei[0], ei[1], np.ones(w.size), (n, n))
    absw = csr(ei[0], ei[1], np.abs(w), (n, n))
    pos, neg = a.copy(), a.copy()
    pos.data = (np.abs(a.data) + a.data) / 2
    neg.data = (np.abs(a.data) - a.data) / 2
    cols = [np.asarray(pos.sum(1)).ravel(), np.asarray(neg.sum(1)).ravel(),
            np.asarray(pos.sum(0)).ravel(), np.asarray(neg.sum(0)).ravel()]
    bounds = []
    for axis in (1, 0):                           # row sums ("in"), then column sums ("out")
        sum_abs = np.asarray(absw.sum(axis)).ravel()
        nnz_u = np.bincount((a.tocoo().row if axis == 1 else a.tocoo().col), minlength=n)
        d = dup.tocoo()
        h_dup = np.zeros(n, dtype=np.int64)
        np.maximum.at(h_dup, d.row if axis == 1 else d.col, team_height(d.data.astype(np.int64)))
        b = np.zeros(n) if exact else gamma(team_height(nnz_u) + h_dup) * sum_abs + ei.shape[1] * E52 * sum_abs
        bounds += [b, b]
    return np.stack(cols, 1), np.stack(bounds, 1)


def check_degree(what, got, want, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    err = np.abs(got - want)
    bad = np.flatnonzero(err > bound)
    if bad.size:
        k = bad[0]
        raise AssertionError(f"{what}: {bad.size} degrees beyond the bar; first [{k // want.shape[1]}, "
                             f"{k % want.shape[1]}] got {got.flat[k]!r} want {want.flat[k]!r} bar {bound.flat[k]:.3g}")
    scale = np.maximum(np.abs(want), 1e-300)
    return float((err / scale).max(initial=0) / U)


# -------------------------------------------------------------------------------------------------------------- second
def transition(ei, n, w):
    """P = D^-1 (A + I) in float64 (existing loops kept, n more appended; deg 0 -> row of zeros), as COO slots, and the
    per-row entry counts (what the device's float32 team sum of deg runs over)."""
    ei = np.asarray(ei, dtype=np.int64)
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    r = np.concatenate([ei[0], np.arange(n)])
    c = np.concatenate([ei[1], np.arange(n)])
    ww = np.concatenate([w, np.ones(n)])
    deg = np.bincount(r, weights=ww, minlength=n)
    sum_abs = np.bincount(r, weights=np.abs(ww), minlength=n)
    inv = np.where(deg != 0, 1.0 / np.where(deg != 0, deg, 1.0), 0.0)
    return r, c, inv[r] * ww, np.bincount(r, minlength=n), deg, sum_abs, bool(np.all(ww == np.round(ww)))


def second_ref(ei, n, w=None):
    """get_second_directed_adj in float64: P, L_in = P^T P, L_out = P P^T, v = (L_in + L_out) / 2 where both are
    non-zero and the sum is non-zero, d = row sums of v, out = d_i^-1/2 v_ij d_j^-1/2.

    The device's roundings, for non-negative weights (every sum below has non-negative terms, so relative bounds
    compose):
      pi_k   P's entries of row k: float32 deg (gamma_h(len_k)), 1/deg in float64, float32(w / deg): u + gamma_h + 3 2^-53
      L_in   sum_k P_ki P_kj: each term off by 2 pi_k, then one rounding of a float64 sum: u + (m + 2) 2^-52
      L_out  sum_k P_ik P_jk: each term off by pi_i + pi_j, then the same rounding
      v      (a + b) * 0.5 in float64, rounded once: u + (err_a + err_b) / (a + b)
      d_i    float32 team sum of row i of v: gamma_h(row length) + the v errors, weighted
      x_i    powf(d_i, -0.5f): half of d's relative error + POWF_ULP ulp (2u per ulp)
      out    (x_i * v) * x_j in float32: 2u
    Typical rows (lengths below 16) come to ~25-30u; the bar is this sum per element, times SECOND_ORDER, plus 2^-30
    for the float64 pipeline of the arbiter itself (<= 2^16 terms per sum at 2^-53 each).
    The same sums bound signed weights, with magnitudes in place of values (sum|t| for every sum that can cancel).
    Returns (Ref, margin, undetermined): the Ref's positions are every one where terms of both products land; `margin` is how far
    L_in, L_out and their sum stand clear of their error bounds (an element with margin <= 1 may be present on one side
    only: pass it as check_elements' cancel_on, the Ref's cancel being 1); `undetermined`: per node, its row sum d is
    within half its own error bound of zero, so the sign of d (NaN or not) or d = 0 is not determined -- elements in
    such a row or column are left out of the value checks (pass ~undetermined[row] & ~undetermined[col] as `held`)."""
    r, c, p, plen, deg, sum_abs_deg, ints = transition(ei, n, w)
    pi = U + gamma(0 if ints else team_height(plen)) * sum_abs_deg / np.where(deg != 0, np.abs(deg), 1.0) + 3 * U64
    P = csr(r, c, p, (n, n))
    absP = csr(r, c, np.abs(p), (n, n))
    cnt = csr(r, c, np.ones(r.size), (n, n))
    abs_in, abs_out = (absP.T @ absP).tocsr(), (absP @ absP.T).tocsr()
    row, col, _ = pattern(abs_in.multiply(abs_out != 0))          # every position where terms of both land
    a, b = at(P.T @ P, row, col), at(P @ P.T, row, col)
    sa, sb = at(abs_in, row, col), at(abs_out, row, col)
    ma, mb = at(cnt.T @ cnt, row, col), at(cnt @ cnt.T, row, col)
    err_a = (at(absP.T @ sp.diags(2 * pi) @ absP, row, col) + U * np.abs(a) + (ma + 2) * E52 * sa) * SECOND_ORDER
    err_b = ((pi[row] + pi[col]) * sb + U * np.abs(b) + (mb + 2) * E52 * sb) * SECOND_ORDER
    v = np.where((a != 0) & (b != 0), (a + b) / 2, 0.0)
    # presence: L_in, L_out and their sum must each be clear of their error bounds (margin > 1), else it may cancel
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.minimum(np.minimum(np.abs(a) / err_a, np.abs(b) / err_b), np.abs(a + b) / (err_a + err_b))
    margin = np.nan_to_num(margin, nan=0.0, posinf=np.inf)
    # v's absolute error: one rounding and the products' errors; where L_in or L_out may be 0 on one side only the mask
    # [L != 0] itself may differ, so the element may be anything up to (|a| + |b|) / 2 on the other
    err_v = U * np.abs(v) + (err_a + err_b) / 2 + np.where(margin <= 1, (np.abs(a) + np.abs(b)) / 2, 0.0)
    d = np.bincount(row, weights=v, minlength=n)
    vabs = np.bincount(row, weights=np.abs(v), minlength=n)
    vlen = np.bincount(row, weights=(margin > 1).astype(np.float64) + (margin <= 1), minlength=n)
    rel_d = (gamma(team_height(vlen.astype(np.int64))) * (vabs + np.bincount(row, weights=err_v, minlength=n)) +
             np.bincount(row, weights=err_v, minlength=n)) / np.where(d != 0, np.abs(d), 1.0)
    with np.errstate(divide="ignore"):
        dis = np.power(d, -0.5)
    dis[np.isinf(dis)] = 0
    out = dis[row] * v * dis[col]
    # d_i^-1/2 from a d_i off by at most rel_d_i, through powf (POWF_ULP ulp): within a factor (1 + F_i) of dis_i, with
    # F_i = (1 - rel_d_i)^-1/2 (1 + 2 POWF_ULP u) - 1 (exact, not first order: rel_d may be large for signed weights);
    # the two float32 products add G = (1 + u)^2 - 1; v itself is off by err_v, so
    # |out_dev - out| <= dis_i dis_j ((|v| + err_v) ((1 + F_i)(1 + F_j)(1 + G) - 1) + err_v)
    with np.errstate(invalid="ignore"):
        F = np.where(rel_d < 1, (1 - np.minimum(rel_d, 1 - 1e-12)) ** -0.5 * (1 + 2 * POWF_ULP * U) - 1, np.inf)
    G = (1 + U) ** 2 - 1
    grow = (1 + F[row]) * (1 + F[col]) * (1 + G) - 1
    bound = ((np.abs(v) + err_v) * grow + err_v) * dis[row] * dis[col] * SECOND_ORDER + 2.0 ** -30 * np.abs(out)
    undetermined = (vabs > 0) & ((d == 0) | (rel_d >= 0.5))          # d's sign or magnitude not determined
    return Ref(n, row, col, out, bound, np.ones(row.size), False), margin, undetermined


# ------------------------------------------------------------------------------------------------------------- checker
def check_elements(what, index, value, ref: Ref, cancel_on=None, held=None):
    """Holds a device CSR (int64 [2, nnz] row-major index, values) to `ref`, element by element:
    - the index is strictly row-major and every entry sits where some term lands;
    - an element with |value| > cancel must be present (exact: every non-zero one, and no zero one);
    - a present element is within `bound` of the float64 value.
    cancel_on: the magnitudes the cancellation rule reads (default ref.val).
    held: per Ref position, whether its value (and NaN-ness) is checked (default all); structure is always checked.
    Returns the worst |got - want| / |want| in units of u (for the record)."""
    index = np.asarray(index, dtype=np.int64).reshape(2, -1)
    value = np.asarray(value, dtype=np.float64).ravel()
    width = max(ref.n_cols, 1)
    keys = index[0] * width + index[1]
    assert keys.size == value.size, f"{what}: {keys.size} indices, {value.size} values"
    assert np.all(np.diff(keys) > 0), f"{what}: index not strictly row-major"
    ref_keys = ref.row * width + ref.col
    pos = np.searchsorted(ref_keys, keys)
    inside = pos < ref_keys.size
    inside[inside] = ref_keys[pos[inside]] == keys[inside]
    if not inside.all():
        k = np.flatnonzero(~inside)[0]
        raise AssertionError(f"{what}: entry ({index[0, k]}, {index[1, k]}) = {value[k]!r} where no term lands")
    present = np.zeros(ref_keys.size, dtype=bool)
    present[pos] = True
    mag = np.abs(ref.val if cancel_on is None else cancel_on)
    must = mag != 0 if ref.exact else mag > ref.cancel
    missing = np.flatnonzero(must & ~present)
    if missing.size:
        k = missing[0]
        raise AssertionError(f"{what}: {missing.size} entries missing; first ({ref.row[k]}, {ref.col[k]}) "
                             f"want {ref.val[k]!r} (cancellation bound {ref.cancel[k]:.3g})")
    if ref.exact:
        extra = np.flatnonzero(present & (mag == 0))
        assert not extra.size, f"{what}: ({ref.row[extra[0]]}, {ref.col[extra[0]]}) present though its sum is 0"
    keep = np.ones(pos.size, bool) if held is None else np.asarray(held)[pos]
    index, value, pos = index[:, keep], value[keep], pos[keep]
    want, bound = ref.val[pos], ref.bound[pos]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(value), nan), f"{what}: NaN pattern differs from float64"
    value, want, bound, pos = value[~nan], want[~nan], bound[~nan], pos[~nan]
    index = index[:, ~nan]
    err = np.abs(value - want)
    bad = np.flatnonzero(err > bound)
    if bad.size:
        k = bad[0]
        raise AssertionError(f"{what}: {bad.size} values beyond the bar; first ({index[0, k]}, {index[1, k]}) got "
                             f"{value[k]!r} want {want[k]!r} |d| = {err[k] / max(abs(want[k]), 1e-300) / U:.3g} u, "
                             f"bar {bound[k] / max(abs(want[k]), 1e-300) / U:.3g} u")
    clear = must[pos]                                         # the record leaves out elements that may cancel
    return float((err[clear] / np.abs(want[clear])).max(initial=0) / U)
