"""Float64 oracle of BSS-eval SDR, SIR and SAR (include/rtfs_amd.h, "BSS-eval SIR and SAR"): the three time-domain ratios of
mir_eval.separation.bss_eval_sources, written from the published definition in numpy / scipy on top of tests/bss_oracle.py (signals,
the scalar projection, the permutation search).  mir_eval itself is not installed where this project is developed, so agreement with
the package is not measured.

``eval_def`` is the definition taken literally: direct correlations, a dense solve of the (J 512)^2 block-Toeplitz system (least
squares when it is singular), the explicit convolutions s_target = s_j * c_j and P_all e = sum_i s_i * C_i of length L + 511, and the
time-domain energies of s_target, e_interf = P_all e - s_target and e_artif = e_pad - P_all e.  ``eval_moments`` is the cheap route the
device takes: the closed forms p_j = c_j'd_j, p_all = C'D_all.  ``block_levinson`` restates the device's joint solver, stop rule
included.  tests/test_bss_eval_host.py holds them together over every case set of the GPU tests."""
import functools

import numpy as np
import scipy.linalg

from tests import bss_oracle as O

F = O.F
STOP = 2.0 ** -46
EDGE_LENGTHS = (1536, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
COND_PAIRS = (("white", "white"), ("ar1_0.9", "ar2_res"), ("ar1_0.99", "butter4_3k"))
COND_LEVELS = (10.0, 30.0, 60.0)  # dB: the interferer's share of the estimate and the noise floor


# ---------------------------------------------------------------- moments
def cross_correlations(S):
    """S (J, L) -> R (512, J, J) with R[k][i][j] = r_ij[k] = sum_t s_i[t] s_j[t+k], k = 0 .. 511; r_ij[-k] = r_ji[k] = R[k][j][i]"""
    S = np.asarray(S, np.float64)
    J, L = S.shape
    R = np.zeros((F, J, J))
    for k in range(min(F, L)):
        R[k] = S[:, :L - k] @ S[:, k:].T
    return R


def right_hand_side(S, e):
    """D (512, J) with D[k][i] = d_i[k] = sum_t s_i[t] e[t+k]"""
    S, e = np.asarray(S, np.float64), np.asarray(e, np.float64)
    L = S.shape[1]
    D = np.zeros((F, S.shape[0]))
    for k in range(min(F, L)):
        D[k] = S[:, :L - k] @ e[k:]
    return D


def dense_gram(R):
    """the (J 512)^2 matrix in tap-major order: G[(a,i),(b,j)] = r_ij[a - b]"""
    J = R.shape[1]
    full = np.concatenate([R[:0:-1].transpose(0, 2, 1), R])  # lags -511 .. 511
    idx = np.subtract.outer(np.arange(F), np.arange(F)) + F - 1
    return full[idx].transpose(0, 2, 1, 3).reshape(F * J, F * J)


def _solve(G, d):
    try:
        c = np.linalg.solve(G, d)
        if not np.isfinite(c).all():
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        c = np.linalg.lstsq(G, d, rcond=None)[0]
    return c


def _active(S):
    """the joint set: the sources that are not silent"""
    return [i for i in range(len(S)) if np.dot(S[i].astype(np.float64), S[i].astype(np.float64)) > 0]


def joint_taps(S, e, solver=None):
    """C (512, J): the taps of the joint projection of e onto the 512 delayed copies of every source of S; a silent source has taps 0"""
    S = np.asarray(S, np.float64)
    act = _active(S)
    C = np.zeros((F, len(S)))
    if act:
        R, D = cross_correlations(S[act]), right_hand_side(S[act], e)
        if solver is None:
            C[:, act] = _solve(dense_gram(R), D.reshape(-1)).reshape(F, len(act))
        else:
            C[:, act] = solver(R, D[:, :, None])[0][:, :, 0]
    return C


def _ratio(num, den):
    return O._db(num, den)


# ---------------------------------------------------------------- the joint solver of the device, restated
def _inverse(E, floor):
    """Gauss-Jordan without pivoting on a J x J error block -> (inverse, ok); ok is False when a pivot is not above its floor"""
    J = len(E)
    A, I = np.array(E, np.float64), np.eye(J)
    for i in range(J):
        p = A[i, i]
        if not p > floor[i]:
            return I, False
        A[i], I[i] = A[i] * (1.0 / p), I[i] * (1.0 / p)
        for k in range(J):
            if k != i:
                f = A[k, i]
                A[k], I[k] = A[k] - f * A[i], I[k] - f * I[i]
    return I, True


def block_levinson(R, Y):
    """Block Levinson for the symmetric block-Toeplitz system with blocks R[a - b] (R[-k] = R[k]'), right-hand sides Y (512, J, q) ->
    (C (512, J, q), order).  Forward and backward block predictors, the error blocks E_f and E_b inverted by Gauss-Jordan without
    pivoting.  Stop rule: the recursion ends at order m when a pivot of either error block of that order is not above 2^-46 r_ii[0];
    taps m .. 511 stay 0.  A source with r_ii[0] = 0 is decoupled (its diagonal entry is set to 1): its taps come out 0."""
    R = np.array(R, np.float64)
    J, q = R.shape[1], Y.shape[2]
    floor = np.array([R[0][i][i] * STOP for i in range(J)])
    for i in range(J):
        if R[0][i][i] == 0:
            R[0][i][i] = 1.0
    C = np.zeros((F, J, q))
    Ef = Eb = R[0]
    Ei, ok = _inverse(R[0], floor)
    if not ok:
        return C, 0
    Eif = Eib = Ei
    Fw, Bw = np.zeros((F, J, J)), np.zeros((F, J, J))
    Fw[0] = Bw[0] = np.eye(J)
    C[0] = Ei @ Y[0]
    for m in range(1, F):
        delta = sum(R[m - t] @ Fw[t] for t in range(m))
        eta = sum(R[m - t] @ C[t] for t in range(m))
        Kf, Kb = Eib @ delta, Eif @ delta.T
        Efn, Ebn = Ef - delta.T @ Kf, Eb - delta @ Kb
        inv_f, ok_f = _inverse(Efn, floor)
        inv_b, ok_b = _inverse(Ebn, floor)
        if not (ok_f and ok_b):
            return C, m
        shifted = np.concatenate([np.zeros((1, J, J)), Bw[:m]])  # [0; B]
        Fn = Fw[:m + 1] - shifted @ Kf
        Bn = shifted - Fw[:m + 1] @ Kb
        Fw[:m + 1], Bw[:m + 1] = Fn, Bn
        C[:m + 1] += Bn @ (inv_b @ (Y[m] - eta))
        Ef, Eb, Eif, Eib = Efn, Ebn, inv_f, inv_b
    return C, F


# ---------------------------------------------------------------- the figures of one (estimate, source) pair
def _convolve(S, C):
    return sum(np.convolve(np.asarray(S[i], np.float64), C[:, i]) for i in range(len(S)))


def figures_def(S, j, e, C=None):
    """(SDR, SIR, SAR) of estimate e against source j of the span S (J, L), the definition: explicit convolutions, time-domain energies"""
    S = np.asarray(S, np.float64)
    r, d, _ = O.correlations(S[j], e)
    c = _solve(scipy.linalg.toeplitz(r), d) if r[0] > 0 else np.zeros(F)
    target = np.convolve(S[j], c)
    e_pad = np.zeros(len(target))
    e_pad[:len(e)] = e
    proj = _convolve(S, joint_taps(S, e) if C is None else C)
    interf, artif = proj - target, e_pad - proj
    tt = np.dot(target, target)
    return (_ratio(tt, np.dot(e_pad - target, e_pad - target)), _ratio(tt, np.dot(interf, interf)),
            _ratio(np.dot(proj, proj), np.dot(artif, artif)))


def figures_moments(S, j, e, C=None, solver=None):
    """the same from the closed forms: p_j = c_j'd_j, p_all = C'D_all, ee"""
    S = np.asarray(S, np.float64)
    r, d, ee = O.correlations(S[j], e)
    p_j = float(np.dot(scipy.linalg.solve_toeplitz(r, d), d)) if r[0] > 0 else 0.0
    act = _active(S)
    if len(act) == 1:  # the joint set is one source: P_all is its scalar projection (the device takes that solve's value)
        ra, da, _ = O.correlations(S[act[0]], e)
        p_all = float(np.dot(scipy.linalg.solve_toeplitz(ra, da), da))
    else:
        if C is None:
            C = joint_taps(S, e, solver)
        p_all = float(np.sum(C * right_hand_side(S, e)))
    return (_ratio(p_j, max(ee - p_j, 0.0)), _ratio(p_j, max(p_all - p_j, 0.0)), _ratio(p_all, max(ee - p_all, 0.0)))


def _evaluate(fn, clean, est, others, mix, perm_by):
    if perm_by not in ("sdr", "sir"):
        raise ValueError(perm_by)
    n = len(clean)
    S = np.concatenate([clean, others]) if others is not None and len(others) else np.asarray(clean)
    taps = [joint_taps(S, est[i]) for i in range(n)]  # one joint solve per estimate
    M = [[fn(S, j, est[i], taps[i]) for j in range(n)] for i in range(n)]
    perm = O.best_perm([[M[i][j][0 if perm_by == "sdr" else 1] for j in range(n)] for i in range(n)])
    sdr, sir, sar = (np.array([M[perm[j]][j][k] for j in range(n)]) for k in range(3))
    sdr_i = None
    if mix is not None:
        with np.errstate(invalid="ignore"):
            sdr_i = sdr - np.array([O.sdr_lu(clean[j], mix) if fn is figures_def else O.sdr_moments(clean[j], mix) for j in range(n)])
    return sdr, sir, sar, sdr_i, perm


def eval_def(clean, est, others=None, mix=None, perm_by="sdr"):
    """clean, est (n, L), others (m, L) | None, mix (L) | None -> (sdr, sir, sar (n), sdr_i (n) | None, perm (n)) in float64, by the
    definition.  perm[j] = the estimate assigned to clean source j; sar[j] is the SAR of that estimate."""
    return _evaluate(figures_def, clean, est, others, mix, perm_by)


def eval_moments(clean, est, others=None, mix=None, perm_by="sdr"):
    return _evaluate(figures_moments, clean, est, others, mix, perm_by)


# ---------------------------------------------------------------- cases (float32, as the device reads them)
@functools.lru_cache(maxsize=None)
def edge_case(L):
    """(clean (1,L), est (1,L), others (1,L)) with J = 2: an AR(1) 0.9 target, a white interferer 10 dB below it in the estimate, white
    noise 20 dB below"""
    rng = np.random.default_rng(5000 + L)
    s, o = O.coloured(rng, L, "ar1_0.9"), O.coloured(rng, L, "white")
    e = (s + np.float32(0.316) * o + np.float32(0.1) * O.coloured(rng, L, "white")).astype(np.float32)
    return s[None], e[None], o[None]


@functools.lru_cache(maxsize=None)
def cond_case(pair, level):
    """(clean (1,L), est (1,L), others (1,L)) at L = 8193: target coloured COND_PAIRS[pair][0], interferer [1], the estimate = target +
    interferer at -level dB + white noise at -level dB: SIR and SAR near `level`"""
    a, b = COND_PAIRS[pair]
    rng = np.random.default_rng(6000 + 10 * pair + int(level))
    s, o = O.coloured(rng, O.COND_L, a), O.coloured(rng, O.COND_L, b)
    g = np.float32(10.0 ** (-level / 20.0))
    e = (s + g * o + g * O.coloured(rng, O.COND_L, "white")).astype(np.float32)
    return s[None], e[None], o[None]


@functools.lru_cache(maxsize=None)
def others_case(m):
    """(clean (1,L), est (1,L), others (m,L)) at L = 4097: n = 1 with m other sources leaking into the estimate at -10 - 5 i dB"""
    rng = np.random.default_rng(7000 + m)
    L = O.SOURCES_L
    s = O.coloured(rng, L, "ar1_0.9")
    others = np.stack([O.coloured(rng, L, O.REFERENCES[(i + 2) % 5]) for i in range(m)])
    e = s + np.float32(0.05) * O.coloured(rng, L, "white")
    for i in range(m):
        e = e + np.float32(10.0 ** (-(10 + 5 * i) / 20.0)) * others[i]
    return s[None], e.astype(np.float32)[None], others


@functools.lru_cache(maxsize=None)
def sir_perm_case():
    """(clean (2,L), est (2,L)) at L = 8192 on which the two permutation rules differ.  e_0 = s_0 + 0.5 s_1 (nearly clean), e_1 = s_0 +
    0.35 s_1 + white noise at 1.5.  The noise is artefact: it lowers both SDRs of e_1 alike and leaves its SIRs alone.  So by SDR e_0
    keeps source 0 (means -3.5 against -7.5 dB), while by SIR e_1, which holds less of s_1 than e_0 does, takes it (1.0 against 0.5 dB)."""
    rng = np.random.default_rng(8000)
    L = 8192
    s0, s1 = O.coloured(rng, L, "ar1_0.9"), O.coloured(rng, L, "white")
    e0 = (s0 + np.float32(0.5) * s1 + np.float32(0.05) * O.coloured(rng, L, "white")).astype(np.float32)
    e1 = (s0 + np.float32(0.35) * s1 + np.float32(1.5) * O.coloured(rng, L, "white")).astype(np.float32)
    return np.stack([s0, s1]), np.stack([e0, e1])


def regular_cases():
    """{name: (clean, est, others | None, mix | None)}: every case the GPU tests compare against ``eval_def``"""
    out = {}
    for L in EDGE_LENGTHS:
        out[f"edge_L{L}"] = edge_case(L) + (None,)
    for n in (2, 3, 4):
        for identical in ((False, True) if n == 2 else (False,)):
            clean, est, mix, _ = O.source_case(n, identical)
            out[f"src{n}{'i' if identical else ''}"] = (clean, est, None, mix)
    for m in (1, 3):
        out[f"others{m}"] = others_case(m) + (None,)
    for p in range(len(COND_PAIRS)):
        for level in COND_LEVELS:
            out[f"cond{p}_{level:g}"] = cond_case(p, level) + (None,)
    return out
