"""Numpy restatement of the host arithmetic behind a different number of faces per mixture (AVNet.separate_speakers(counts=...),
AVNet.separate_many_speakers, rtfs_longform_many_speakers_plan), built on tests/many_oracle.py.  Nothing here imports the package under
test.

The target-to-mixture table: targets are mixture-major, mix_of[t] = the mixture of target t, non-decreasing.

The pooled plan: recording r has K_r lip tracks and N_r windows.  Window rows lie in recording order, then window order (row0, as in
many_oracle); target rows lie the same way with the K_r targets of a window side by side: trow0[r] = sum of N_q K_q before r, target row
= trow0[r] + n K_r + k.  Recording r's (K_r, L_r) result starts off[r] floats into one flat output, every block rounded up to 32 floats.

The chunks: consecutive windows whose targets total at most max_batch; a window with more targets than max_batch goes alone."""
from tests import longform_oracle as LO
from tests import many_oracle as MO

MAX_K = 16
INT32_MAX = 2 ** 31 - 1


def mix_of(counts):
    return [b for b, c in enumerate(counts) for _ in range(int(c))]


def plan(Ls, Tvs, Ks, window, hop=None):
    """dict(row0, N, L, Tv, off, K, trow0: lists of R ints; rows = sum(N); targets = sum(N K); floats = size of the flat output)."""
    Ls, Tvs, Ks = [int(v) for v in Ls], [int(v) for v in Tvs], [int(v) for v in Ks]
    if len(Ls) < 1 or len(Ls) != len(Tvs) or len(Ls) != len(Ks):
        raise ValueError(f"{len(Ls)} lengths, {len(Tvs)} video lengths, {len(Ks)} track counts")
    row0, N, off, trow0 = [], [], [], []
    rows = targets = floats = 0
    for L, Tv, K in zip(Ls, Tvs, Ks):
        if L > INT32_MAX or Tv > INT32_MAX:
            raise ValueError(f"L = {L}, Tv = {Tv} past int32")
        if not 1 <= K <= MAX_K:
            raise ValueError(f"K = {K}")
        n = LO.plan(L, Tv, window, hop)
        row0.append(rows)
        trow0.append(targets)
        N.append(n)
        off.append(floats)
        rows += n
        targets += n * K
        floats += -(-K * L // MO.ALIGN) * MO.ALIGN
    if rows > INT32_MAX or targets > INT32_MAX:
        raise ValueError(f"{rows} windows, {targets} targets past int32")
    return dict(row0=row0, N=N, L=Ls, Tv=Tvs, off=off, K=Ks, trow0=trow0, rows=rows, targets=targets, floats=floats)


def table(p):
    """The 7 * R words [row0 | N | L | Tv | off | K | trow0] of a plan."""
    return p["row0"] + p["N"] + p["L"] + p["Tv"] + p["off"] + p["K"] + p["trow0"]


def window_counts(p):
    """Targets of every window, in row order."""
    return [K for K, n in zip(p["K"], p["N"]) for _ in range(n)]


def chunks(counts, max_batch):
    """[(w0, w1, t0, t1)]: windows [w0, w1) = target rows [t0, t1)."""
    out, w, t = [], 0, 0
    while w < len(counts):
        w1, n = w + 1, counts[w]
        while w1 < len(counts) and n + counts[w1] <= max_batch:
            n += counts[w1]
            w1 += 1
        out.append((w, w1, t, t + n))
        w, t = w1, t + n
    return out
