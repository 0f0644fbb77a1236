"""A NumPy model of `dtype = f32`: the same operation as the kernels, with the roundings the design documents
and no others.  It gives the mode a reference of its own: the error of the model against the fp64 oracle, over a sample of
null-space bases, is the fp32 rounding budget of one case, and the engine is held to a small multiple of it.

  stack(prob, ref, rng)    the oracle's accepted blocks [H_o | r_o], each in a random orthonormal basis of its null space.  The
                           basis is free (the engine's Householder basis is not the oracle's SVD basis) and what fp32 rounding does
                           depends on it, so the model samples it.  The gate is not modelled: it runs in fp64 before anything is
                           rounded, the accepted mask is the oracle's.
  update(stack, P, ...)    round_stack: the stack through fp32 (k_feature stores [H_o | r_o] as float).  Then MSCKF.py:594-598 as
                           the oracle does them, and the sequential 16-row block update of DESIGN.md 3.3 on the state augmented by
                           the dx row.  round_products: the subtracted term X_I X_I^T formed in fp32 from fp32 operands and widened;
                           P itself stays fp64 (`dtype = f32`).
  budget(prob, ref, ...)   the largest deviation from the oracle over S samples, as rel_err on dx and P+.
  budget_measures(...)     the same in the five measures of `filter_prior.metrics`: rel_err on dx and P+, scaled_dx, scaled_P,
                           update_term -- what a filter-shaped prior needs to be read in.
  chain_update(stack, ..)  the K6-K7 chain (`launch_gain`, msckf_abi.hip): the only update of windows of 83 - 221 clones, the retry
                           after a timeout and the path under MSCKF_GAIN_STREAM=0.  T, r_n, Y, S, K, dx in fp64; P+ from the three
                           Joseph products on `k_gemm_f32` and `k_symmetrize_f32`, in fp32 from the load of P to the last store.
  chain_budget_measures    its budget, in the five measures.
  bound_measures(b)        what the engine is held to in each of them.

Outside the model, on the flat tolerance: the chain at d = 1137 - 1341 (chain_187, chain_221, the `few` cases of
tests/filter_prior.py), where sixteen samples of the model are minutes of CPU, and the two cases that miss a condition of
tests/test_f32_filter_prior.py (test_gpu_f32_filter_prior.OUTSIDE).
CPU only, plain fp64 / fp32 NumPy."""
import numpy as np

from conftest import rel_err

# The engine's error is one more draw from the population the S = 16 samples come from: both are sums of very many independent
# fp32 roundings under a random basis.  The maximum of 16 draws sits near mean + 1.8 sigma; 4 times that maximum is out of reach
# of a correct kernel and well inside what a lost term or a misplaced tile does (tests/test_f32_model.py).  Chosen before the
# first GPU run, measured against the model and never against the engine's own output.
MARGIN = 4

FLAT_DX, FLAT_P = 1e-4, 1e-5          # the mode's flat tolerance (tests/test_gpu_f32.py); the budget only ever tightens it


def blocks(prob, ref):
    """[H_o | r_o] (q x (d + 1)) of every feature the oracle accepted, in the oracle's basis."""
    from oracle import msckf_oracle as oracle
    out = []
    for j in np.nonzero(np.asarray(ref["accepted"]))[0]:
        r, H_x, H_f = oracle.feature_blocks(prob, int(j))
        r_o, H_o = oracle.project_on_nullspace(H_f, r, H_x)
        out.append(np.hstack([H_o, r_o[:, None]]))
    return out


def stack(prob, ref, rng, blks=None):
    """The stacked [H_X | r_o] in fp64, every block multiplied from the left by a random orthogonal q x q matrix (QR of a
    Gaussian matrix from `rng`).  `blks`: blocks(prob, ref), when the caller draws more than one sample."""
    blks = blocks(prob, ref) if blks is None else blks
    d = prob.P.shape[0]
    if not blks:
        return np.zeros((0, d + 1))
    out = []
    for B in blks:
        q = B.shape[0]
        Q, R = np.linalg.qr(rng.standard_normal((q, q)))
        out.append((Q * np.sign(np.diag(R))) @ B)            # (Haar: the sign fix of the QR's column freedom)
    return np.vstack(out)


def exact_product(Xa, I):
    return Xa @ Xa.T


def f32_product(Xa, I):
    """v_mfma_f32_16x16x4_f32: fp32 operands, fp32 sums of 16 terms, widened before the fp64 subtraction."""
    X32 = Xa.astype(np.float32)
    return (X32 @ X32.T).astype(np.float64)


def row_blocks(m):
    """Blocks of 16 rows; when m is no multiple of 16 the SHORT block is the first ("Beside the sweep")."""
    first = m % 16
    edges = ([0, first] if first else [0]) + list(range(first + 16, m + 1, 16))
    return list(zip(edges[:-1], edges[1:]))


def update(stk, P, sigma, round_stack, round_products, product=None):
    """(dx, P+) of the stacked system `stk` = [H_X | r_o] against P.  `product(Xa, I)`: the term block I subtracts from the
    augmented covariance, for tests that inject a defect; the default is the exact or the fp32 product."""
    d = P.shape[0]
    if product is None:
        product = f32_product if round_products else exact_product
    if round_stack:
        stk = stk.astype(np.float32).astype(np.float64)
    if stk.shape[0] > d:                                     # MSCKF.py:594-598: T_H = R, r_n = Q^T r_o -- the R factor of
        R = np.linalg.qr(stk, mode="r")                      # [H_X | r_o] holds both, and Q (m x d) is never formed
        T, r_n = R[:d, :d], R[:d, d]
    else:                                                    # :599-602
        T, r_n = stk[:, :d], stk[:, d]
    Pa = np.zeros((d + 1, d + 1))                            # the state augmented by one row that ends as -dx
    Pa[:d, :d] = (P + P.T) / 2                               # the input symmetrised as it is loaded
    for I, (a, b) in enumerate(row_blocks(T.shape[0])):
        T_I, r_I = T[a:b], r_n[a:b]
        Ya = Pa[:, :d] @ T_I.T                               # Y_I = P^(I) T_I^T
        Ya[d] += r_I
        A = T_I @ Ya[:d] + sigma ** 2 * np.eye(b - a)        # A_I = T_I Y_I + sigma^2 I
        L = np.linalg.cholesky(A)
        Xa = np.linalg.solve(L, Ya.T).T                      # X_I = Y_I L_II^-T
        Pa -= product(Xa, I)                                 # P^(I+1) = P^(I) - X_I X_I^T
    return -Pa[d, :d].copy(), Pa[:d, :d].copy()


def budget(prob, ref, products, S=16, seed=0, first=0, blks=None):
    """(max_s e_dx, max_s e_P, per-sample array (S, 2)) of samples first .. first + S - 1: the model with the stack rounded
    (and the products, if `products`) against the oracle's dx and P+."""
    b, per = budget_measures(prob, ref, products, S=S, seed=seed, first=first, blks=blks)
    return b[0], b[1], per[:, :2]


def _measures(prob, ref, model, S, seed, first, blks, diag_min):
    from filter_prior import metrics
    blks = blocks(prob, ref) if blks is None else blks
    per = np.zeros((S, 5))
    for s in range(S):
        rng = np.random.default_rng([seed, first + s])
        dx, Pn = model(stack(prob, ref, rng, blks))
        per[s] = metrics(dx, Pn, ref, prob.P)
        if diag_min is not None:
            diag_min.append(float(np.diag(Pn).min()))
    return tuple(float(x) for x in per.max(axis=0)), per


def budget_measures(prob, ref, products, S=16, seed=0, first=0, blks=None, diag_min=None):
    """`budget` in the five measures of `filter_prior.metrics`: ((max_s e_dx, e_P, s_dx, s_P, u_P), per-sample array (S, 5)).
    diag_min: a list that receives min(diag(P+)) of every sample."""
    return _measures(prob, ref, lambda stk: update(stk, prob.P, prob.sigma, True, products), S, seed, first, blks, diag_min)


def budget_sequence(probs, refs, products, S=16, seed=0, first=0, diag_min=None):
    """Consecutive updates with the covariance committed in between: probs[k] was built on the ORACLE's P after step k - 1,
    every sample of the model carries its own rounded P through the steps.  Per step k: the five maxima of
    `filter_prior.metrics` (the first two: max_s e_dx, max_s e_P) against the oracle after k + 1 steps, the prior of the scaled
    measures being the oracle's probs[k].P, and the per-sample array (steps, S, 5)."""
    from filter_prior import metrics
    blks = [blocks(p, r) for p, r in zip(probs, refs)]
    per = np.zeros((len(probs), S, 5))
    for s in range(S):
        rng = np.random.default_rng([seed, first + s])
        P = probs[0].P
        for k, (p, r) in enumerate(zip(probs, refs)):
            dx, P = update(stack(p, r, rng, blks[k]), P, p.sigma, True, products)
            per[k, s] = metrics(dx, P, r, p.P)
            if diag_min is not None:
                diag_min.append(float(np.diag(P).min()))
    return [tuple(float(x) for x in per[k].max(axis=0)) for k in range(len(probs))], per


def bound(b_dx, b_P):
    """What the engine is held to: the budget times MARGIN, never wider than the mode's flat tolerance."""
    return min(FLAT_DX, MARGIN * b_dx), min(FLAT_P, MARGIN * b_P)


FLAT_SCALED = 1e-4                    # a condition on the cases, not a measurement: a budget in covariance units whose bound
#                                       reached a ten-thousandth of a sigma would no longer say anything (tests/test_f32_filter_prior.py)


def bound_measures(b):
    """`bound` in the five measures: MARGIN * b, capped by the flat pair on the two rel_err columns and by FLAT_SCALED on
    scaled_dx, scaled_P and update_term."""
    caps = (FLAT_DX, FLAT_P, FLAT_SCALED, FLAT_SCALED, FLAT_SCALED)
    return tuple(min(c, MARGIN * float(x)) for c, x in zip(caps, b))


# ---- the chain ------------------------------------------------------------------------------------------------------------------

GEMM_WAVES = 8                        # k_gain.h, MSCKF_GEMM_WAVES: the wavefronts that share the K range of one 16 x 16 tile


def gemm_f32(A, B, C0, alpha, beta, tri=False, operand=None):
    """`k_gemm_f32` with transB: float32(alpha * A B^T + beta * C0), A (M x K), B (N x K), C0 (M x N).
    Every operand is fp32 as it is loaded (`ld32`: the fp64 P, K, Y, T are rounded there, the update's own B2, D, Pn are fp32
    already), alpha and beta are floats, the accumulator is fp32 and is never widened: v_mfma_f32_16x16x4_f32 over the
    K range cut into GEMM_WAVES contiguous pieces, the partial tiles summed in fp32 in wavefront order, then alpha, then
    beta * C0, then the fp32 store.  tri: B is upper triangular and the tiles of columns n0 .. n0 + 15 start at k = n0.
    (Within a piece the order of the fp32 sum is NumPy's, not the matrix core's: the same roundings in another order.)
    `operand(name, X32)`: a defect injected into the fp32 operand "A" or "B" (tests)."""
    A32, B32 = np.asarray(A).astype(np.float32), np.asarray(B).astype(np.float32)
    if operand is not None:
        A32, B32 = operand("A", A32), operand("B", B32)
    M, K = A32.shape
    N = B32.shape[0]
    out = np.zeros((M, N), dtype=np.float32)
    for n0 in (range(0, N, 16) if tri else [0]):
        cols = slice(n0, min(n0 + 16, N)) if tri else slice(0, N)
        kbeg = n0 if tri else 0
        kq = -(-(K - kbeg) // (4 * GEMM_WAVES))
        x = np.zeros((M, cols.stop - cols.start), dtype=np.float32)
        for w in range(GEMM_WAVES):
            ks = slice(min(kbeg + 4 * kq * w, K), min(kbeg + 4 * kq * (w + 1), K))
            x = x + A32[:, ks] @ B32[cols, ks].T
        out[:, cols] = x
    out = (out * np.float32(alpha)).astype(np.float64)       # x += beta * c0 is one fused multiply-add (-ffp-contract=on)
    return (out + np.float64(np.float32(beta)) * np.asarray(C0).astype(np.float32).astype(np.float64)).astype(np.float32)


def chain_update(stk, P, sigma, round_stack, round_joseph, operand=None):
    """(dx, P+) of the stacked system `stk` = [H_X | r_o] against P on the chain (`launch_gain`).  T and r_n are the R factor of
    the (rounded) stack's clone columns -- always reduced: the chain's second product relies on a triangular T -- and
    Y = P[:, 15:] T^T, S = T Y[15:] + sigma^2 I, K = Y S^-1, dx = K r_n are fp64, as the chain forms them in either dtype.
    round_joseph: P+ from `launch_gain`'s f32 branch,
        B2 = P - K Y^T,   D = (float) sigma^2 K - B2[:, 15:] T^T,   Pn = B2 + D K^T   on `gemm_f32`,   P+ = 0.5f (Pn + Pn^T),
    fp32 from the load of P to `k_symmetrize_f32`'s sum, widened at its store.  Otherwise the same three products in fp64.
    `operand(product, name, X32)`: a defect in one fp32 operand of product 0, 1 or 2 (tests)."""
    d = P.shape[0]
    assert not stk[:, :15].any()                             # the IMU columns of H_X are zero: T_H = [0 | T]
    if round_stack:
        stk = stk.astype(np.float32).astype(np.float64)
    R = np.linalg.qr(stk[:, 15:], mode="r")[:d - 15]
    T, r_n = R[:, :d - 15], R[:, d - 15]
    P = (P + P.T) / 2
    s2 = sigma ** 2
    Y = P[:, 15:] @ T.T
    S = T @ Y[15:] + s2 * np.eye(T.shape[0])
    K = np.linalg.solve(S, Y.T).T
    dx = K @ r_n
    if not round_joseph:
        B2 = P - K @ Y.T
        D = s2 * K - B2[:, 15:] @ T.T
        Pn = B2 + D @ K.T
        return dx, (Pn + Pn.T) / 2
    op = lambda i: None if operand is None else (lambda name, X: operand(i, name, X))
    B2 = gemm_f32(K, Y, P, -1.0, 1.0, operand=op(0))
    D = gemm_f32(B2[:, 15:], T, K, -1.0, s2, tri=True, operand=op(1))
    Pn = gemm_f32(D, K, B2, 1.0, 1.0, operand=op(2))
    return dx, (np.float32(0.5) * (Pn + Pn.T)).astype(np.float64)


def chain_budget_measures(prob, ref, S=16, seed=0, first=0, blks=None, diag_min=None):
    """`budget_measures` of the chain: stack and Joseph products rounded."""
    return _measures(prob, ref, lambda stk: chain_update(stk, prob.P, prob.sigma, True, True), S, seed, first, blks, diag_min)
