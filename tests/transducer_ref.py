"""Checker for the transducer kernels (csrc/transducer.hip): float64 references of the targets, the joint, the lattice loss and every
gradient, a float32 evaluation of the kernels' arithmetic, a reference greedy decoder, and the case table.  Never imported by the
product.

Conventions (include/amdspeech.h, "transducer"): f [T][B][J], g [U+1][B][J] time-major, lattice tensors [B][T][U+1][C], blank C-1,
T_b = min(max(lengths[b], 0), T), node (b, t, u) live when t < T_b and u <= n_b.

The stages are checked ONE BY ONE on the same float32 inputs: the joint on f / g / W_out, the loss on the float32 rounding of the
reference's logits, the joint's backward on the float32 rounding of the reference's dlogits.  The float64 gradient of the loss comes
from autograd through a plain loop over the lattice's anti-diagonals (loss_ref); tests/test_cpu_transducer.py holds that loop
against brute-force enumeration of every alignment and against finite differences.

Bounds.  None comes from a GPU but one constant: E_TANH, the relative error of the device's tanhf.  lm_ref.E_LIBM = 4 documents exp
and log only, and no figure for tanhf is written down for this device, so it was MEASURED once: the joint kernel with J = C = 16, the
identity as W_out, g = 0 and b_out = 0 returns its own tanhf(f) exactly; over 2^20 arguments in [-20, 20] (half of them uniform there,
a quarter each in [-1, 1] and [-4, 4]) the largest error against float64 was 2.46 u relative (8.4e-8 absolute, at x = 0.65).  E_TANH is
that measurement with a factor 2, rounded up: 5 u.  u = 2**-24; expf / logf within E = lm_ref.E_LIBM u as everywhere in the suite.

loss, dlogits   as tests/ctc_ref.py: the bound of a slice (an utterance's loss; 16 frames of an utterance's dlogits) is FACTOR = 8
                times the error of the emulated arithmetic against float64 ON THAT SLICE, not below a floor of a few float32
                roundings (LOSS_FLOOR, D_FLOOR), never looser than LOSS_CAP = 2e-5 relative / D_CAP = 2e-3 absolute.  A row of
                dlogits sums to zero within rowsum_bound (C more roundings).
                The recursion state is float64 on the device.  ctc_ref.py records why CTC went there: |alpha| grows by ~ 5 units per
                frame with random logits, one float32 rounding of alpha at T + U ~ 500 is 3e-5 .. 6e-5, and alpha + beta - ln P adds
                three of them in the exponent of every gradient term.  `state32_errors` repeats the emulation with a float32 state:
                at the table's sizes it is harmless, at the workload's diagonal count the same arithmetic that put CTC over its cap
                applies, and a float64 logaddexp per node is not what bounds the loss call (the row kernels are).
logits          z_k = tanh(fl(f + g)): |dz_k| <= u |f + g| + E_TANH u |z_k| = e_z.  A (J + 1)-term sum of products in any order:
                    e_logit = sum_bound(J + 1, (|z| + e_z) . |W| + |b|) + e_z . |W|.
df, dg, dW, db  dzp = dlogits . W^T: C terms; dz = dzp (1 - z^2): + 3 u |dz| + 2 |z| e_z |dzp|;  then sums over the live u (df), the
                live t (dg), the live nodes (dW: products z dlogits, + e_z |dlogits|; db).  Every sum, in ANY order and grouping
                (tiles, partials, second pass), is inside sum_bound(n, sum |terms|) with n its term count.  The bound of an element is
                max(FACTOR x emulation error on the tensor, that formula).
"""
import functools
import itertools

import numpy as np
import torch

import lm_ref as R
from oracle import model as om

F32, F64 = np.float32, np.float64
U_RND = R.U
E = R.E_LIBM
E_TANH = 5.0                 # MEASURED on the GPU (2.46 u) x 2, rounded up: module docstring
FACTOR = 8.0
LOSS_CAP, D_CAP = 2e-5, 2e-3
D_FLOOR = 2.0 ** -21          # softmax, the three occupancy terms and their differences: a few float32 roundings of magnitude <= 1
LOSS_FLOOR = 2.0 ** -22       # the loss is one float32 rounding of a float64 sum of float32 log-probabilities
FAULTS = ("wrong_terminal", "label_at_end", "missing_gamma")
T_BLOCK = 16


# ---------------------------------------------------------------------------------------------------------------- targets
def targets_ref(dense, C):
    """dense int [B, U] -> (targets [B, U] zero-padded, n [B], tok [B, U+2], tok_len [B]): zeros dropped, the target is every kept
    label before the first one >= C-1; an empty target is a valid row.  Negative ids are dropped with the zeros."""
    dense = np.asarray(dense)
    B, U = dense.shape
    targets = np.zeros((B, U), np.int32)
    n = np.zeros(B, np.int32)
    tok = np.full((B, U + 2), C - 1, np.int32)
    for b in range(B):
        kept = []
        for v in dense[b]:
            if v <= 0:                      # (the padding, and ids that are no label)
                continue
            if v >= C - 1:
                break
            kept.append(int(v))
        n[b] = len(kept)
        targets[b, :len(kept)] = kept
        tok[b, 1:1 + len(kept)] = kept
    return targets, n, tok, (n + 1).astype(np.int32)


def live_mask(lengths, n, T, U):
    """bool [B, T, U+1]."""
    Tb = np.clip(np.asarray(lengths), 0, T)
    return (np.arange(T)[None, :, None] < Tb[:, None, None]) & (np.arange(U + 1)[None, None, :] <= np.asarray(n)[:, None, None])


# ---------------------------------------------------------------------------------------------------------------- joint
def joint_ref(f, g, w, bias):
    """float64 logits [B, T, U+1, C] on every node."""
    f, g, w, bias = (np.asarray(x, F64) for x in (f, g, w, bias))
    z = np.tanh(f.transpose(1, 0, 2)[:, :, None, :] + g.transpose(1, 0, 2)[:, None, :, :])
    return z @ w + bias


def joint_bound(f, g, w, bias):
    """e_logit of the module docstring, [B, T, U+1, C]."""
    f, g, w, bias = (np.asarray(x, F64) for x in (f, g, w, bias))
    s = f.transpose(1, 0, 2)[:, :, None, :] + g.transpose(1, 0, 2)[:, None, :, :]
    z = np.abs(np.tanh(s))
    ez = U_RND * np.abs(s) + E_TANH * U_RND * z
    J = w.shape[0]
    return R.sum_bound(J + 1, (z + ez) @ np.abs(w) + np.abs(bias)) + ez @ np.abs(w)


def joint_f32(f, g, w, bias):
    f, g, w, bias = (np.asarray(x, F32) for x in (f, g, w, bias))
    z = np.tanh(f.transpose(1, 0, 2)[:, :, None, :] + g.transpose(1, 0, 2)[:, None, :, :]).astype(F32)
    return (z @ w + bias).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- loss
def _lattice_loss_torch(lp, y, Tb, nb, blank):
    """-ln P of one utterance: lp [Tb, nb+1, C] log-probabilities (torch float64), a plain walk over the anti-diagonals."""
    lpb = lp[:, :, blank]
    alpha = torch.full((Tb, nb + 1), -np.inf, dtype=lp.dtype)
    alpha = alpha.index_put((torch.tensor([0]), torch.tensor([0])), torch.zeros(1, dtype=lp.dtype))
    yi = torch.as_tensor(np.asarray(y[:nb], np.int64))
    for d in range(1, Tb + nb):
        us = np.arange(max(0, d - Tb + 1), min(nb, d) + 1)
        ts = d - us
        vals = []
        for t, u in zip(ts, us):
            terms = []
            if t > 0:
                terms.append(alpha[t - 1, u] + lpb[t - 1, u])
            if u > 0:
                terms.append(alpha[t, u - 1] + lp[t, u - 1, yi[u - 1]])
            vals.append(terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1]))
        alpha = alpha.index_put((torch.as_tensor(ts), torch.as_tensor(us)), torch.stack(vals))
    return -(alpha[Tb - 1, nb] + lpb[Tb - 1, nb])


def loss_ref(logits, targets, n, lengths):
    """float64 (loss [B], dlogits [B, T, U+1, C] = d(sum loss)/dlogits) on the given logits (taken as float64); dead nodes and rows
    with T_b = 0 get zeros."""
    x = torch.tensor(np.asarray(logits, F64), requires_grad=True)
    B, T, U1, C = x.shape
    losses = []
    for b in range(B):
        Tb, nb = int(np.clip(lengths[b], 0, T)), int(n[b])
        if Tb == 0:
            losses.append(torch.zeros((), dtype=torch.float64))
            continue
        lp = torch.log_softmax(x[b, :Tb, :nb + 1], dim=-1)
        losses.append(_lattice_loss_torch(lp, targets[b], Tb, nb, C - 1))
    total = torch.stack(losses).sum()
    if total.requires_grad:
        total.backward()
    d = x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    return np.array([float(l.detach()) for l in losses]), d


def brute_force_loss(lp, y, blank):
    """-ln of the sum over EVERY alignment: lp [T, n+1, C] float64 log-probabilities.  An alignment is an order of T blanks and n
    labels whose last move is a blank (the terminal one); the node of a move is (blanks so far, labels so far)."""
    T, n1, _ = lp.shape
    n = n1 - 1
    total = []
    for pos in itertools.combinations(range(T - 1 + n), n):      # where the labels sit among the first T - 1 + n moves
        t = u = 0
        s = 0.0
        for i in range(T - 1 + n):
            if i in pos:
                s += lp[t, u, y[u]]; u += 1
            else:
                s += lp[t, u, blank]; t += 1
        total.append(s + lp[T - 1, n, blank])
    total = np.array(total)
    m = total.max()
    return -(m + np.log(np.exp(total - m).sum()))


def log_softmax32(x):
    x = np.asarray(x, F32)
    m = x.max(axis=-1, keepdims=True)
    d = (x - m).astype(F32)
    s = np.exp(d).astype(F32).sum(axis=-1, keepdims=True, dtype=F32)
    return (d - np.log(s).astype(F32)).astype(F32), d, np.log(s).astype(F32)


def _lae(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(hi), hi, hi + np.log1p(np.exp(lo - hi)))


def emulate_loss(logits, targets, n, lengths, fault=None, state=F64):
    """The kernels' arithmetic on the CPU: log-softmax in float32, alpha / beta with a `state` recursion on the float32
    log-probabilities, the three occupancy terms in float64 rounded once to float32, the gradient row in float32.  `fault` plants
    one of FAULTS."""
    x = np.asarray(logits, F32)
    B, T, U1, C = x.shape
    loss = np.zeros(B, F32)
    d = np.zeros(x.shape, F32)
    for b in range(B):
        Tb, nb = int(np.clip(lengths[b], 0, T)), int(n[b])
        if Tb == 0:
            continue
        lp, dd, logs = log_softmax32(x[b, :Tb, :nb + 1])
        p = np.exp((dd - logs).astype(F32)).astype(F32)
        lpb = lp[:, :, C - 1].astype(state)
        y = np.asarray(targets[b][:nb], np.int64)
        lpy = np.full((Tb, nb + 1), -np.inf, state)
        if nb:
            lpy[:, :nb] = np.take_along_axis(lp[:, :nb], y[None, :, None], axis=2)[:, :, 0]
        al = np.full((Tb, nb + 1), -np.inf, state)
        be = np.full((Tb, nb + 1), -np.inf, state)
        al[0, 0] = 0.0
        for t in range(Tb):
            for u in range(nb + 1):
                if t == 0 and u == 0:
                    continue
                a1 = al[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
                a2 = al[t, u - 1] + lpy[t, u - 1] if u > 0 else -np.inf
                al[t, u] = state(_lae(state(a1), state(a2)))
        tt, tu = (Tb - 1, nb) if fault != "wrong_terminal" else (Tb - 1, max(nb - 1, 0))
        be[Tb - 1, nb] = lpb[Tb - 1, nb]
        for t in range(Tb - 1, -1, -1):
            for u in range(nb, -1, -1):
                if t == Tb - 1 and u == nb:
                    continue
                b1 = be[t + 1, u] + lpb[t, u] if t + 1 < Tb else -np.inf
                b2 = be[t, u + 1] + lpy[t, u] if u < nb else -np.inf
                be[t, u] = state(_lae(state(b1), state(b2)))
        lnp = F64(al[tt, tu]) + F64(lpb[tt, tu])
        loss[b] = F32(-lnp)
        al64, be64 = al.astype(F64), be.astype(F64)
        bt = np.full((Tb, nb + 1), -np.inf)
        bt[:-1] = be64[1:]
        bt[Tb - 1, nb] = 0.0                                   # beta past the terminal node
        bu = np.full((Tb, nb + 1), -np.inf)
        bu[:, :nb] = be64[:, 1:]
        gam = np.exp(al64 + be64 - lnp).astype(F32)
        if fault == "missing_gamma":
            gam = np.ones_like(gam)
        eb = np.exp(al64 + lpb.astype(F64) + bt - lnp).astype(F32)
        ey = np.zeros((Tb, nb + 1), F32)
        if nb:
            ey[:, :nb] = np.exp(al64[:, :nb] + lpy[:, :nb].astype(F64) + bu[:, :nb] - lnp).astype(F32)
        row = (p * gam[:, :, None]).astype(F32)
        row[:, :, C - 1] -= eb
        for u in range(nb):
            row[:, u, y[u]] -= ey[:, u]
        if fault == "label_at_end" and nb:                     # the label term applied at u = n_b as well
            row[:, nb, y[nb - 1]] -= np.exp(al64[:, nb] + lp[:, nb, y[nb - 1]].astype(F64) + be64[:, nb] - lnp).astype(F32)
        d[b, :Tb, :nb + 1] = row
    return loss, d


def frame_blocks(Tb):
    return [(t0, min(t0 + T_BLOCK, Tb)) for t0 in range(0, Tb, T_BLOCK)]


def slice_errors(got_loss, got_d, ref_loss, ref_d, lengths):
    """-> {("loss", b): relative error, ("d", b, t0, t1): max abs error}."""
    B, T = ref_d.shape[:2]
    out = {}
    gl, rl = np.asarray(got_loss, F64), np.asarray(ref_loss, F64)
    gd, rd = np.asarray(got_d, F64), np.asarray(ref_d, F64)
    for b in range(B):
        if not np.isfinite(gl[b]):
            out[("loss", b)] = np.inf
        else:
            out[("loss", b)] = abs(gl[b] - rl[b]) / abs(rl[b]) if rl[b] != 0 else abs(gl[b])
        for t0, t1 in frame_blocks(int(np.clip(lengths[b], 0, T))):
            e = np.abs(gd[b, t0:t1] - rd[b, t0:t1])
            out[("d", b, t0, t1)] = float(np.inf if np.isnan(e).any() else e.max())
    return out


def loss_bounds(emu_errors):
    return {k: min(LOSS_CAP, FACTOR * max(e, LOSS_FLOOR)) if k[0] == "loss" else min(D_CAP, FACTOR * max(e, D_FLOOR))
            for k, e in emu_errors.items()}


def rowsum_worst(d, live):
    s = np.abs(np.asarray(d, F64).sum(axis=-1))
    return float(s[live].max()) if live.any() else 0.0


def rowsum_bound(emu_worst, C):
    """The row sum adds C float32 values of magnitude <= 1 to the slice's floor; else 8 x the emulation's, capped."""
    return min(D_CAP, FACTOR * max(emu_worst, D_FLOOR + C * 2.0 ** -24))


# ---------------------------------------------------------------------------------------------------------------- joint, backward
def joint_bwd_ref(dl, f, g, w, live):
    """float64 (df, dg, dw, db) of the live nodes' dlogits, and their bounds (same shapes) by the module docstring's formulas."""
    dl, f, g, w = (np.asarray(x, F64) for x in (dl, f, g, w))
    m = live[..., None]
    dl = np.where(m, dl, 0.0)
    s = f.transpose(1, 0, 2)[:, :, None, :] + g.transpose(1, 0, 2)[:, None, :, :]
    z = np.tanh(s)
    ez = U_RND * np.abs(s) + E_TANH * U_RND * np.abs(z)
    C = w.shape[1]
    dzp = dl @ w.T
    dzp_abs = np.abs(dl) @ np.abs(w).T
    dz = dzp * (1 - z * z)
    e_dz = R.sum_bound(C, dzp_abs) + 3 * U_RND * np.abs(dz) + 2 * np.abs(z) * ez * np.abs(dzp)
    n_u = live.sum(axis=2)[..., None].astype(F64)                      # [B, T, 1]
    n_t = live.sum(axis=1)[..., None].astype(F64)                      # [B, U1, 1]
    df = dz.sum(axis=2).transpose(1, 0, 2)
    e_df = (e_dz.sum(axis=2) + R.sum_bound(n_u, (np.abs(dz) + e_dz).sum(axis=2))).transpose(1, 0, 2)
    dg = dz.sum(axis=1).transpose(1, 0, 2)
    e_dg = (e_dz.sum(axis=1) + R.sum_bound(n_t, (np.abs(dz) + e_dz).sum(axis=1))).transpose(1, 0, 2)
    nn = float(max(live.sum(), 1))
    zl = np.where(m, z, 0.0).reshape(-1, z.shape[-1])
    ezl = np.where(m, ez, 0.0).reshape(-1, z.shape[-1])
    dlf = dl.reshape(-1, C)
    dw = zl.T @ dlf
    e_dw = R.sum_bound(nn + 1, (np.abs(zl) + ezl).T @ np.abs(dlf)) + ezl.T @ np.abs(dlf)
    db = dlf.sum(axis=0)
    e_db = R.sum_bound(nn + 1, np.abs(dlf).sum(axis=0))
    return (df, dg, dw, db), (e_df, e_dg, e_dw, e_db)


def joint_bwd_f32(dl, f, g, w, live):
    dl, f, g, w = (np.asarray(x, F32) for x in (dl, f, g, w))
    m = live[..., None]
    dl = np.where(m, dl, F32(0))
    z = np.tanh(f.transpose(1, 0, 2)[:, :, None, :] + g.transpose(1, 0, 2)[:, None, :, :]).astype(F32)
    dz = ((dl @ w.T).astype(F32) * (F32(1) - z * z)).astype(F32)
    zl = np.where(m, z, F32(0)).reshape(-1, z.shape[-1])
    return (dz.sum(axis=2, dtype=F32).transpose(1, 0, 2), dz.sum(axis=1, dtype=F32).transpose(1, 0, 2),
            (zl.T @ dl.reshape(-1, dl.shape[-1])).astype(F32), dl.reshape(-1, dl.shape[-1]).sum(axis=0, dtype=F32))


def joint_bwd_bounds(formula, emu, ref):
    """Per element: max(FACTOR x the emulation's largest error on the tensor, the formula)."""
    return tuple(np.maximum(FACTOR * float(np.abs(np.asarray(e, F64) - r).max()), fb) for fb, e, r in zip(formula, emu, ref))


# ---------------------------------------------------------------------------------------------------------------- the case table
U_TILE_CLASSES = ((5, 16), (80, 16), (81, 48), (256, 16))      # (C, J): one class count of every instantiation of the joint kernels
REC_U_EDGES = ((63, "wave"), (64, "block1"), (255, "block1"), (256, "block4"), (1023, "block4"), (1024, "block10"))


def row(length, n, rep=False):
    return dict(length=length, n=n, rep=rep)


def case(name, T, U, J, C, rows, scale=1.0, seed=0):
    return dict(name=name, T=T, U=U, J=J, C=C, rows=rows, B=len(rows), scale=scale, seed=seed)


def cases(plan):
    """The smallest shapes at which each kernel can go wrong, from `plan(T, B, U, J, C)` (ops.rnnt_plan): T of 1, 2 and either side
    of the frame tile and of the backward's frame chunk; n_b of 0, 1, U and either side of every prefix tile and of every recursion
    kernel; B of 1, 3, 33 with ragged lengths (0, T, T + 5); J of 16, 48 and the largest; C of 2, 5, 80, 81, 256; repeated labels; a
    large logit scale."""
    p = plan(5, 3, 80, 16, 5)
    tt, fu, bu, tc = p["fwd_t_tile"], p["fwd_u_tile"], p["bwd_u_tile"], p["bwd_t_chunk"]
    assert (tt, bu, tc) == (p["bwd_t_tile"], 16, 32), p
    out = [
        case("t1", 1, 3, 16, 5, [row(1, 3)]),
        case("t2-ragged", 2, 4, 48, 5, [row(2, 0), row(0, 1), row(7, 4)]),
        case("t-tile", tt + 1, bu + 1, 16, 80, [row(tt, bu - 1, True), row(tt + 1, bu), row(tt + 6, bu + 1, True)]),
        case("t-chunk", tc + 1, 6, 48, 81, [row(tc, 6), row(tc + 1, 1), row(tc + 6, 0)]),
        case("b33", 6, 5, 16, 256, [row((7 * i) % 12, (3 * i) % 6, i % 2 == 1) for i in range(33)]),
        case("j-max", 5, 3, plan(5, 1, 3, 16, 80)["j_max"], 80, [row(5, 2)]),
        case("c2", 4, 2, 16, 2, [row(4, 0), row(0, 0), row(9, 0)]),
        case("large", 9, 7, 48, 80, [row(9, 7, True), row(5, 3), row(14, 0)], scale=12.0),
    ]
    # either side of the forward's prefix tile OF EVERY INSTANTIATION (the tile is 64, 64, 32, 16 wide by class count): n_b = tile - 2
    # and tile - 1 end inside the first tile, n_b = tile and tile + 1 reach the second; the backward walks its 16-wide steps on the way
    for C, J in U_TILE_CLASSES:
        fu = plan(3, 3, 4, J, C)["fwd_u_tile"]
        assert plan(3, 3, fu + 1, J, C)["fwd_u_tiles"] == 2 and fu + 2 > bu, (C, fu)
        out.append(case("u-tile-c%d" % C, 3, fu + 1, J, C, [row(2, fu - 1, True), row(3, fu), row(1, fu + 1)]))
        out.append(case("u-tile-low-c%d" % C, 3, fu + 1, J, C, [row(3, fu - 2)]))
    for U, kern in REC_U_EDGES:
        assert plan(2, 1, U, 16, 5)["rec_kernel"] == kern, (U, kern)
        out.append(case("rec-%d" % U, 2 if U > 64 else 4, U, 16, 5, [row(4, U, U < 100)]))
    return out


def build(c):
    """The arrays of a case: float32 f, g, w, b, int32 dense labels and lengths; the targets by targets_ref."""
    rng = np.random.RandomState(1000 + c["seed"] + 7 * c["T"] + 13 * c["U"] + c["J"] + c["C"])
    T, U, J, C, B = c["T"], c["U"], c["J"], c["C"], c["B"]
    f = rng.randn(T, B, J).astype(F32)
    g = rng.randn(U + 1, B, J).astype(F32)
    w = (rng.randn(J, C) * c["scale"] / np.sqrt(J)).astype(F32)
    bias = (rng.randn(C) * 0.1).astype(F32)
    dense = np.zeros((B, U), np.int32)
    for b, r in enumerate(c["rows"]):
        n = r["n"] if C > 2 else 0
        y = rng.randint(1, max(C - 1, 2), size=n)
        if r["rep"] and n >= 2:
            y[1::2] = y[0:-1:2][:len(y[1::2])]
        dense[b, :n] = y
        if n < U:
            dense[b, n] = C - 1
    lengths = np.array([r["length"] for r in c["rows"]], np.int32)
    targets, n, tok, tok_len = targets_ref(dense, C)
    assert C == 2 or list(n) == [r["n"] for r in c["rows"]]
    return dict(f=f, g=g, w=w, bias=bias, dense=dense, lengths=lengths, targets=targets, n=n, tok=tok, tok_len=tok_len,
                live=live_mask(lengths, n, T, U))


@functools.lru_cache(maxsize=None)
def evaluated(name, plan):
    """Everything a test needs of a case, computed once: the inputs, the float64 references stage by stage, the emulations and
    the bounds."""
    c = {k["name"]: k for k in cases(plan)}[name]
    a = build(c)
    ev = dict(case=c, **a)
    ev["logits_ref"] = joint_ref(a["f"], a["g"], a["w"], a["bias"])
    ev["logits_bound"] = joint_bound(a["f"], a["g"], a["w"], a["bias"])
    ev["logits_emu"] = joint_f32(a["f"], a["g"], a["w"], a["bias"])
    x32 = np.where(a["live"][..., None], ev["logits_ref"], 0.0).astype(F32)
    ev["logits32"] = x32
    ev["loss_ref"], ev["d_ref"] = loss_ref(x32, a["targets"], a["n"], a["lengths"])
    el, ed = emulate_loss(x32, a["targets"], a["n"], a["lengths"])
    ev["emu_errors"] = slice_errors(el, ed, ev["loss_ref"], ev["d_ref"], a["lengths"])
    ev["bounds"] = loss_bounds(ev["emu_errors"])
    ev["rowsum_bound"] = rowsum_bound(rowsum_worst(ed, a["live"]), c["C"])
    ev["emu_loss"], ev["emu_d"] = el, ed
    d32 = ev["d_ref"].astype(F32)
    ev["d32"] = d32
    ev["bwd_ref"], formula = joint_bwd_ref(d32, a["f"], a["g"], a["w"], a["live"])
    ev["bwd_emu"] = joint_bwd_f32(d32, a["f"], a["g"], a["w"], a["live"])
    ev["bwd_bounds"] = joint_bwd_bounds(formula, ev["bwd_emu"], ev["bwd_ref"])
    return ev


def state32_errors(name, plan):
    ev = evaluated(name, plan)
    el, ed = emulate_loss(ev["logits32"], ev["targets"], ev["n"], ev["lengths"], state=F32)
    return slice_errors(el, ed, ev["loss_ref"], ev["d_ref"], ev["lengths"])


def judge(ev, got_loss, got_d):
    """The slices of (got_loss, got_d) over their bound: [] when the case passes."""
    err = slice_errors(got_loss, got_d, ev["loss_ref"], ev["d_ref"], ev["lengths"])
    return [(k, e, ev["bounds"][k]) for k, e in sorted(err.items(), key=str) if not e <= ev["bounds"][k]]


# ---------------------------------------------------------------------------------------------------------------- greedy decoding
def pred_params(L, H, V, J, seed=0):
    """float32 parameters of a prediction network (the language model's names, oracle.model's initialisation) and its projection."""
    p = om.init_params(L, H, V, V, seed=2000 + seed)
    rng = np.random.RandomState(seed)
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(F32)
    p["pred_w"] = (rng.randn(H, J) / np.sqrt(H)).astype(F32)
    p["pred_b"] = (rng.randn(J) * 0.1).astype(F32)
    return p


def greedy_walk(p, L, f, lengths, U, w, bias, step, dtype=F64, forced=None):
    """Time-synchronous greedy decoding in `dtype`: `step(p, L, h, c, token) -> (h', c', _)` is lm_fusion_ref.lm_step_ref (float64)
    or lm_step_f32.  `forced` (the `choices` of an earlier walk) replays that walk's decisions instead of taking the argmax.
    Returns (ids [B, U] zero-padded, out_len [B], choices: per row the class taken at every node visited, rows: per row the logit
    row of every node visited)."""
    f, w, bias = (np.asarray(x, dtype) for x in (f, w, bias))
    pw, pb = np.asarray(p["pred_w"], dtype), np.asarray(p["pred_b"], dtype)
    T, B, J = f.shape
    C = w.shape[1]
    H = pw.shape[0]
    ids = np.zeros((B, U), np.int32)
    out_len = np.zeros(B, np.int32)
    choices, rows = [], []
    for b in range(B):
        h = np.zeros((1, L, H), dtype); c = np.zeros((1, L, H), dtype)
        h, c, _ = step(p, L, h, c, np.array([C - 1]))
        t = m = 0
        Tb = int(np.clip(lengths[b], 0, T))
        ch, rw = [], []
        while t < Tb and m < U:
            gproj = (np.asarray(h[0, L - 1], dtype) @ pw + pb).astype(dtype)
            lg = (np.tanh(f[t, b] + gproj).astype(dtype) @ w + bias).astype(dtype)
            k = int(np.argmax(lg)) if forced is None else forced[b][len(ch)]
            ch.append(k); rw.append(lg)
            if k == C - 1:
                t += 1
            else:
                ids[b, m] = k; m += 1
                h, c, _ = step(p, L, h, c, np.array([k]))
        out_len[b] = m
        choices.append(ch); rows.append(rw)
    return ids, out_len, choices, rows


def greedy_margins(rows64, rows32):
    """(the smallest top-two margin of the float64 rows, the largest |float32 - float64| logit) over every node visited."""
    margin, err = np.inf, 0.0
    for r64, r32 in zip(rows64, rows32):
        for a, b in zip(r64, r32):
            top = np.sort(a)
            margin = min(margin, float(top[-1] - top[-2]))
            err = max(err, float(np.abs(np.asarray(b, F64) - a).max()))
    return margin, err


GREEDY_LOGIT_FLOOR = 2.0 ** -17      # a logit of magnitude ~ 4 after two matrix products and a recurrent state: tens of float32 roundings


def greedy_logit_bound(emu_err):
    """FACTOR x the float32 walk's largest logit error along the float64 path, not below the floor."""
    return FACTOR * max(emu_err, GREEDY_LOGIT_FLOOR)


GREEDY_CASES = (   # name, L, H, J, C, T, U, lengths, seed, blank bias
    ("mixed", 1, 16, 16, 6, 7, 6, (7, 0, 5), 1, 1.5),
    ("capped", 2, 48, 48, 6, 6, 3, (6, 0, 11), 2, -3.0),      # blank pushed down: rows emit until m = U
    ("blanky", 1, 16, 48, 80, 9, 5, (9, 4, 0), 3, 5.0),
)


def greedy_case(name):
    name, L, H, J, C, T, U, lengths, seed, bb = {c[0]: c for c in GREEDY_CASES}[name]
    rng = np.random.RandomState(300 + seed)
    p = pred_params(L, H, C, J, seed)
    f = rng.randn(T, len(lengths), J).astype(F32)
    w = (rng.randn(J, C) * 2.0 / np.sqrt(J)).astype(F32)
    bias = (rng.randn(C) * 0.1).astype(F32)
    bias[C - 1] += F32(bb)
    return dict(name=name, L=L, H=H, J=J, C=C, T=T, U=U, B=len(lengths), lengths=np.array(lengths, np.int32), p=p, f=f, w=w, bias=bias)
