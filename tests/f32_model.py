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
  budget(prob, ref, ...)   the largest deviation from the oracle over S samples.

Outside the model, on the flat tolerance: the chain's Joseph products on k_gemm_f32 (forced, retry, N > 82) and edge_gauge_prior.
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
    blks = blocks(prob, ref) if blks is None else blks
    per = np.zeros((S, 2))
    for s in range(S):
        rng = np.random.default_rng([seed, first + s])
        dx, Pn = update(stack(prob, ref, rng, blks), prob.P, prob.sigma, True, products)
        per[s] = rel_err(dx, ref["dx"]), rel_err(Pn, ref["P_new"])
    return float(per[:, 0].max()), float(per[:, 1].max()), per


def budget_sequence(probs, refs, products, S=16, seed=0, first=0):
    """Consecutive updates with the covariance committed in between: probs[k] was built on the ORACLE's P after step k - 1,
    every sample of the model carries its own rounded P through the steps.  Per step k: (max_s e_dx, max_s e_P) against the
    oracle after k + 1 steps, and the per-sample array (steps, S, 2)."""
    blks = [blocks(p, r) for p, r in zip(probs, refs)]
    per = np.zeros((len(probs), S, 2))
    for s in range(S):
        rng = np.random.default_rng([seed, first + s])
        P = probs[0].P
        for k, (p, r) in enumerate(zip(probs, refs)):
            dx, P = update(stack(p, r, rng, blks[k]), P, p.sigma, True, products)
            per[k, s] = rel_err(dx, r["dx"]), rel_err(P, r["P_new"])
    return [(float(per[k, :, 0].max()), float(per[k, :, 1].max())) for k in range(len(probs))], per


def bound(b_dx, b_P):
    """What the engine is held to: the budget times MARGIN, never wider than the mode's flat tolerance."""
    return min(FLAT_DX, MARGIN * b_dx), min(FLAT_P, MARGIN * b_P)
