"""Numpy restatement (float64) of the pooled windowing behind AVNet.separate_many, built on tests/longform_oracle.py: every recording is
planned, framed and cross-faded on its own, exactly as DESIGN.md "Long recordings" says; the only new rule is the layout.  Nothing here
imports the package under test.

The sum(N_r) windows lie in recording order, then window order: recording r owns rows [row0[r], row0[r] + N_r), row0[r] = sum of N
before r.  Its (n_src, L_r) result starts off[r] floats into one flat output, every block rounded up to ALIGN = 32 floats (one 128-byte
line): off[r] = sum over q < r of 32 * ceil(n_src * L_q / 32)."""
import numpy as np

from tests import longform_oracle as LO

ALIGN = 32
INT32_MAX = 2 ** 31 - 1


def plan(Ls, Tvs, window, hop=None, n_src=1):
    """dict(row0, N, L, Tv, off: lists of R ints; rows = sum(N); floats = size of the flat output).  ValueError for what the formulas do
    not cover."""
    Ls, Tvs = [int(v) for v in Ls], [int(v) for v in Tvs]
    if len(Ls) < 1 or len(Ls) != len(Tvs) or n_src < 1:
        raise ValueError(f"{len(Ls)} lengths, {len(Tvs)} video lengths, n_src {n_src}")
    row0, N, off = [], [], []
    rows = floats = 0
    for L, Tv in zip(Ls, Tvs):
        if L > INT32_MAX or Tv > INT32_MAX:
            raise ValueError(f"L = {L}, Tv = {Tv} past int32")
        n = LO.plan(L, Tv, window, hop)
        row0.append(rows)
        N.append(n)
        off.append(floats)
        rows += n
        floats += -(-n_src * L // ALIGN) * ALIGN
    if rows > INT32_MAX:
        raise ValueError(f"{rows} windows past int32")
    return dict(row0=row0, N=N, L=Ls, Tv=Tvs, off=off, rows=rows, floats=floats)


def table(p):
    """The 5 * R words [row0 | N | L | Tv | off] of a plan."""
    return p["row0"] + p["N"] + p["L"] + p["Tv"] + p["off"]


def frame(xs, vs, window, hop=None):
    """xs: R arrays (L_r), vs: R arrays (512, Tv_r) -> (sum N, window), (sum N, 512, window / SPF); copies, the dtype is kept."""
    parts = [LO.frame(np.asarray(x)[None], np.asarray(v)[None], window, hop) for x, v in zip(xs, vs)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def overlap_add(y, Ls, window, hop=None):
    """y (sum N, n_src, window) pooled -> R arrays (n_src, L_r) float64, each the longform overlap-add of its own rows."""
    out, row = [], 0
    for L in Ls:
        n = LO.plan(L, 1, window, hop)
        out.append(LO.overlap_add(y[row:row + n], 1, L, window, hop)[0])
        row += n
    assert row == y.shape[0], (row, y.shape)
    return out


def flat(results, p, n_src, fill=np.nan):
    """The R results laid into the flat output of plan p; the padding holds ``fill``."""
    out = np.full(p["floats"], fill, np.float64)
    for res, o, L in zip(results, p["off"], p["L"]):
        out[o:o + n_src * L] = np.asarray(res).reshape(-1)
    return out
