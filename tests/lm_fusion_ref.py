"""Checker for first-pass fusion (csrc/lm_step.hip, the fused decoder of csrc/beam.cpp): the float64 step on oracle.model's
cell, a float32 numpy evaluation of the same step, the rounding bounds as formulas, a dictionary-keyed fused prefix beam search, a
brute-force scorer and the case tables.  Never imported by the product.

Conventions (include/amdspeech.h: amdspeech_lm_step): a row has a parent state h, c [L][H] (zero for parent -1), a token and
produces h', c' [L][H] and logq [V]; parameters under the ParamLayout(L, H, V, V) names.

Rounding bounds, u = 2**-24, E = lm_ref.E_LIBM (libm functions within E u relative), all per element and first order with the
second-order terms covered by sum_bound's 1 / (1 - n u).  Parent states and parameters are the same float32 numbers on both sides.

x_0          fl(input_w[token] + input_b): one rounding, e_x = u |x_0|.
gates        g = [x ; h] . K + b is a (2H + 1)-term sum of products; a fused multiply-add chain in any order satisfies
             lm_ref.sum_bound(2H + 1, sum |a_k K_k| + |b|), and an input error e_x[k] arrives as sum_k e_x[k] |K_k|:
                 e_g = sum_bound(2H + 1, (|x| + e_x ; |h|) . |K| + |b|) + e_x . |K_x|.
             The gate functions have slopes <= 1 and values in [-1, 1]: sigmoid as 1 / (1 + exp(-g)) is within (E + 2) u, tanh
             within E u; f + 1 costs one more rounding u (|g_f| + 1):
                 e_i = e_g + (E + 2) u,  e_j = e_g + E u,  e_f = e_g + u (|g_f| + 1) + (E + 2) u,  e_o = e_g + (E + 2) u.
cell         c' = c f + i j, two products and a sum:  e_c = |c| e_f + e_i + e_j + e_i e_j + 2 u (|c f| + |i j|).
             h' = tanh(c') o:  e_h = e_c + E u + e_o + u.          x of the next layer is h': e_x = e_h.
logits       z = h'_top . W + b, (H + 1) terms:  e_z = sum_bound(H + 1, (|h'| + e_h) . |W| + |b|) + e_h . |W|.
logq         logq_c = z_c - lse(z).  For exact z lm_ref.nll_bound(V, M) bounds lse - z_c (M = max |z|, taken with e_z added); an
             error e_z of the inputs moves lse by at most max e_z and z_c by e_z[c]:
                 e_q = nll_bound(V, M) + e_z + max_v e_z.
"""
import itertools

import numpy as np

import lm_ref as R
from oracle import model as om

U = R.U
E = R.E_LIBM


# ------------------------------------------------------------------------------------------------------------- the step
def _onehot(token, V, dtype):
    token = np.asarray(token)
    x = np.zeros((1, len(token), V), dtype)
    ok = (token >= 0) & (token < V)
    x[0, np.arange(len(token))[ok], token[ok]] = 1.0
    return x


def lm_step_ref(p, L, h, c, token):
    """float64: p a dict of float64 parameters, h / c [N, L, H] the parent states (zero rows for parent -1), token [N] ->
    (h' [N, L, H], c' [N, L, H], logq [N, V]) through oracle.model.forward: one time step, the states handed in."""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    h, c = np.asarray(h, np.float64), np.asarray(c, np.float64)
    N, V = h.shape[0], p["input_w"].shape[0]
    state = [(c[:, l], h[:, l]) for l in range(L)]
    logits, final, _ = om.forward(p, _onehot(token, V, np.float64), np.ones(N, np.int64), L, state=state)
    z = logits[0]
    m = z.max(axis=1, keepdims=True)
    logq = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))
    return np.stack([final[l][1] for l in range(L)], 1), np.stack([final[l][0] for l in range(L)], 1), logq


def lm_step_f32(p, L, h, c, token, variant="right"):
    """The same step in float32 numpy, operation by operation as the kernel does it (the bounds must hold for it), and two
    deliberately WRONG variants the bounds must reject: "no_forget_bias" (sigmoid(f) instead of sigmoid(f + 1)) and
    "neighbour_parent" (row r reads the parent state of row r + 1)."""
    f = np.float32
    p = {k: np.asarray(v, f) for k, v in p.items()}
    h, c = np.asarray(h, f), np.asarray(c, f)
    if variant == "neighbour_parent":
        h, c = np.roll(h, -1, axis=0), np.roll(c, -1, axis=0)
    token = np.asarray(token)
    V, H = p["input_w"].shape
    ok = (token >= 0) & (token < V)
    x = np.where(ok[:, None], p["input_w"][np.where(ok, token, 0)], f(0)) + p["input_b"]
    hs, cs = [], []

    def sig(v):
        return f(1) / (f(1) + np.exp(-v))

    for l in range(L):
        g = np.concatenate([x, h[:, l]], axis=1) @ p["kernel_%d" % l] + p["bias_%d" % l]
        gi, gj, gf, go = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        fb = f(0) if variant == "no_forget_bias" else f(om.FORGET_BIAS)
        cn = c[:, l] * sig(gf + fb) + sig(gi) * np.tanh(gj)
        hn = np.tanh(cn) * sig(go)
        hs.append(hn.astype(f)); cs.append(cn.astype(f))
        x = hs[-1]
    z = (x @ p["output_w"] + p["output_b"]).astype(f)
    m = z.max(axis=1, keepdims=True)
    logq = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True, dtype=f)))
    return np.stack(hs, 1), np.stack(cs, 1), logq.astype(f)


def lm_step_bounds(p, L, h, c, token):
    """(e_h [N, L, H], e_c [N, L, H], e_q [N, V]): the bounds of the module docstring, evaluated on the float64 reference."""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    h, c = np.asarray(h, np.float64), np.asarray(c, np.float64)
    token = np.asarray(token)
    V, H = p["input_w"].shape
    ok = (token >= 0) & (token < V)
    x = np.where(ok[:, None], p["input_w"][np.where(ok, token, 0)], 0.0) + p["input_b"]
    e_x = U * np.abs(x)
    e_hs, e_cs = [], []
    for l in range(L):
        K, b = p["kernel_%d" % l], p["bias_%d" % l]
        a = np.concatenate([x, h[:, l]], axis=1)
        a_abs = np.concatenate([np.abs(x) + e_x, np.abs(h[:, l])], axis=1)
        g = a @ K + b
        e_g = R.sum_bound(2 * H + 1, a_abs @ np.abs(K) + np.abs(b)) + e_x @ np.abs(K[:H])
        gi, gj, gf, go = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        e_i = e_g[:, :H] + (E + 2) * U
        e_j = e_g[:, H:2 * H] + E * U
        e_f = e_g[:, 2 * H:3 * H] + U * (np.abs(gf) + 1.0) + (E + 2) * U
        e_o = e_g[:, 3 * H:] + (E + 2) * U
        i, j, f_, o = om.sigmoid(gi), np.tanh(gj), om.sigmoid(gf + om.FORGET_BIAS), om.sigmoid(go)
        cl = c[:, l]
        e_c = np.abs(cl) * e_f + e_i + e_j + e_i * e_j + 2 * U * (np.abs(cl * f_) + np.abs(i * j))
        e_h = e_c + E * U + e_o + U
        e_hs.append(e_h); e_cs.append(e_c)
        x = np.tanh(cl * f_ + i * j) * o
        e_x = e_h
    W, b = p["output_w"], p["output_b"]
    z = x @ W + b
    e_z = R.sum_bound(H + 1, (np.abs(x) + e_x) @ np.abs(W) + np.abs(b)) + e_x @ np.abs(W)
    M = (np.abs(z) + e_z).max(axis=1, keepdims=True)
    e_q = R.nll_bound(V, M) + e_z + e_z.max(axis=1, keepdims=True)
    return np.stack(e_hs, 1), np.stack(e_cs, 1), e_q


# ----------------------------------------------------------------------------------------------------- step case table
STEP_SHAPES = ((1, 16, 2), (3, 48, 80), (1, 256, 129), (3, 16, 129), (1, 48, 2), (3, 256, 80))      # (L, H, V)
STEP_N_FIXED = (1, 15, 16, 17, 65)
STEP_N_WALK_MAX = 1 << 20           # the walk over the plan's instantiations stops above this N


def step_row_counts(plan):
    """The fixed N of the table plus, for every instantiation the plan query reports, its last N, the first N of the next one and one
    row above its row tile.  `plan(N, L, H, V)` returns a dict with n_min / n_max / row_tile (ops.lm_step_plan)."""
    ns = set(STEP_N_FIXED)
    n = 1
    while n <= STEP_N_WALK_MAX:
        p = plan(n, 1, 16, 2)
        assert p["n_min"] <= n <= p["n_max"], (n, p)
        ns.add(p["row_tile"] + 1)
        if p["n_max"] <= STEP_N_WALK_MAX:
            ns.update((p["n_max"], p["n_max"] + 1))
        n = p["n_max"] + 1
    return sorted(ns)


def step_params(L, H, V, seed=0):
    """float32 parameters: oracle.model's initialisation with biases of size 0.1 (the bias paths do something)."""
    p = om.init_params(L, H, V, V, seed=1000 + seed)
    rng = np.random.RandomState(seed)
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    return p


def step_case(L, H, V, N, seed=0):
    """One call: a pool of n_slots states (random float32), N rows with parent -1 for a quarter of them and parents SHARED by several
    rows for the rest, dest slots a permuted, non-contiguous set disjoint from the parents, tokens in 0 .. V-1 and -- from 15 rows on --
    one token of V (outside the alphabet: the bias alone).  Returns a dict; h_par / c_par [N, L, H] are the gathered parent states."""
    rng = np.random.RandomState(7919 * H + 131 * V + 17 * L + N + seed)
    n_par = max(1, N // 3)
    n_slots = 2 * N + n_par + 5
    perm = rng.permutation(n_slots)
    par_slots, dest = perm[:n_par], perm[n_par:n_par + N].astype(np.int32)
    parent = np.where(rng.rand(N) < 0.25, -1, par_slots[rng.randint(0, n_par, size=N)]).astype(np.int32)
    if N >= 2:
        parent[0], parent[1] = -1, par_slots[0]
    else:
        parent[0] = par_slots[0]              # (a single row from the zero state would not see the forget gate at all)
    token = rng.randint(0, V, size=N).astype(np.int32)
    if N >= 15:
        token[N - 1] = V
    pool_h = (rng.randn(n_slots, L, H) * 0.5).astype(np.float32)
    pool_c = (rng.randn(n_slots, L, H) * 0.5).astype(np.float32)
    live = (parent >= 0)[:, None, None]
    h_par = np.where(live, pool_h[np.maximum(parent, 0)], np.float32(0))
    c_par = np.where(live, pool_c[np.maximum(parent, 0)], np.float32(0))
    return dict(L=L, H=H, V=V, N=N, n_slots=n_slots, parent=parent, token=token, dest=dest, pool_h=pool_h, pool_c=pool_c,
                h_par=h_par, c_par=c_par, params=step_params(L, H, V, seed))


def step_cases(plan):
    return [step_case(L, H, V, N) for L, H, V in STEP_SHAPES for N in step_row_counts(plan)]


# ------------------------------------------------------------------------------------------------- fused beam search
NEG = -np.inf


def _lse(a, b):
    return np.float32(np.logaddexp(a, b)) if (a != NEG or b != NEG) else NEG


def log_posteriors(lg):
    """float32 log-softmax of logits [T, C], the normaliser in float64 as the decoder takes it."""
    return (lg - np.log(np.exp(lg.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)


def fused_prefix_beam_search(lg, blank, width, lm, lm_weight, lm_length_bonus=0.0):
    """The fused prefix beam search restated with a dictionary keyed by whole prefixes (slow and obviously right about WHICH
    candidates are the same prefix), float32 scores.  lm(prefix tuple) -> q [C], the model's log-probabilities of the next token.
    The extension of a prefix by c adds lm_weight * q[c] + lm_length_bonus; blank and repeat transitions add nothing; the final
    score adds lm_weight * q[blank] (the closing EOS, id C - 1 = blank).  Order: (score descending, prefix lexicographic).
    Returns (ranked list of (prefix, final score), gap): gap is the smallest difference, over all frames, between the last
    candidate kept and the first one dropped, and between the first and second final scores."""
    T, C = lg.shape
    f = np.float32
    lp = log_posteriors(lg)
    w, bonus = f(lm_weight), f(lm_length_bonus)
    cache = {}

    def q_of(pre):
        if pre not in cache:
            cache[pre] = np.asarray(lm(pre), f)
        return cache[pre]

    gap = np.inf
    beams = {(): (f(0.0), NEG)}                           # prefix -> (p_blank, p_non_blank)
    for t in range(T):
        nxt = {}
        for pre, (pb, pnb) in sorted(beams.items()):
            tot = _lse(pb, pnb)
            b0, n0 = nxt.get(pre, (NEG, NEG))
            b0 = _lse(b0, tot + lp[t, blank])
            if pre:
                n0 = _lse(n0, pnb + lp[t, pre[-1]])
            nxt[pre] = (b0, n0)
            q = q_of(pre)
            for c in range(C):
                if c == blank:
                    continue
                frm = pb if (pre and pre[-1] == c) else tot
                if frm == NEG:
                    continue
                b1, n1 = nxt.get(pre + (c,), (NEG, NEG))
                nxt[pre + (c,)] = (b1, _lse(n1, f(frm + lp[t, c]) + f(f(w * q[c]) + bonus)))
        order = sorted(((k, v) for k, v in nxt.items() if _lse(*v) != NEG), key=lambda kv: (-_lse(*kv[1]), kv[0]))
        if len(order) > width:
            gap = min(gap, float(_lse(*order[width - 1][1])) - float(_lse(*order[width][1])))
        beams = dict(order[:width])
    final = sorted(((pre, f(_lse(*v) + f(w * q_of(pre)[blank]))) for pre, v in beams.items()), key=lambda kv: (-kv[1], kv[0]))
    if len(final) > 1:
        gap = min(gap, float(final[0][1]) - float(final[1][1]))
    return [(list(pre), float(s)) for pre, s in final], gap


def ctc_log_prob(lp, seq, blank):
    """float64 log p_ctc(seq | lp [T, C]) by the forward recursion (every alignment that collapses to seq; no merging of the
    labels of seq themselves)."""
    T = lp.shape[0]
    ext = [blank]
    for s in seq:
        ext += [s, blank]
    S = len(ext)
    a = np.full(S, NEG)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        n = np.full(S, NEG)
        for s in range(S):
            v = a[s]
            if s >= 1:
                v = np.logaddexp(v, a[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = np.logaddexp(v, a[s - 2])
            n[s] = v + lp[t, ext[s]] if v != NEG else NEG
        a = n
    return float(np.logaddexp(a[S - 1], a[S - 2]) if S > 1 else a[0])


def brute_force_best(lg, blank, lm, lm_weight, lm_length_bonus=0.0):
    """argmax over ALL label sequences of at most T labels of log p_ctc + lm_weight * log p_lm (with the closing EOS) + bonus *
    tokens, float64: (best sequence, its score, the gap to the second best)."""
    T, C = lg.shape
    lp = log_posteriors(lg).astype(np.float64)
    labels = [c for c in range(C) if c != blank]
    scored = []
    for n in range(T + 1):
        for seq in itertools.product(labels, repeat=n):
            s = ctc_log_prob(lp, seq, blank)
            if s == NEG:
                continue
            lm_sum = sum(float(lm(seq[:k])[seq[k]]) for k in range(n)) + float(lm(seq)[blank])
            scored.append((s + lm_weight * lm_sum + lm_length_bonus * n, seq))
    scored.sort(key=lambda e: (-e[0], e[1]))
    return list(scored[0][1]), scored[0][0], scored[0][0] - scored[1][0]


# ---------------------------------------------------------------------------------------------------------- stub models
def hash_lm(C, seed, sharp=1.0):
    """lm(prefix) -> a log-softmax row [C] drawn from a generator seeded by a hash of the WHOLE prefix (and `seed`): any mistake in
    which parent a state came from changes the row."""
    def lm(prefix):
        hsh = 1469598103934665603 ^ (seed * 1099511628211 & 0xFFFFFFFFFFFFFFFF)
        for v in prefix:
            hsh = ((hsh ^ (int(v) + 1)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        z = np.random.RandomState(hsh % (2 ** 32)).randn(C) * sharp
        return (z - np.log(np.exp(z).sum())).astype(np.float32)
    return lm


class StubStepper(object):
    """A `step` for ops.ctc_beam_search_fused around lm(prefix): keeps its own slot -> prefix map and asserts the slot contract on
    every call (dest distinct, inside the pool, never a parent of the same call; a parent is -1 or a slot that holds a prefix)."""

    def __init__(self, lm, C, n_slots):
        self.lm, self.C, self.n_slots = lm, C, n_slots
        self.prefix_of = {}
        self.calls, self.rows, self.root_steps = 0, [], 0

    def __call__(self, parent, token, dest):
        n = len(parent)
        assert n >= 1 and len(token) == n and len(dest) == n
        assert len(set(dest.tolist())) == n, "dest slots repeat"
        assert all(0 <= d < self.n_slots for d in dest), "a dest slot outside the pool"
        assert not set(dest.tolist()) & set(parent.tolist()), "a dest slot is a parent of the same call"
        out = np.empty((n, self.C), np.float32)
        new = {}
        for r in range(n):
            if parent[r] == -1:
                assert token[r] == self.C - 1, "only the root starts from the zero state"
                self.root_steps += 1
                pre = ()
            else:
                assert int(parent[r]) in self.prefix_of, "a parent slot that holds no state"
                assert 0 <= token[r] < self.C - 1
                pre = self.prefix_of[int(parent[r])] + (int(token[r]),)
            new[int(dest[r])] = pre
            out[r] = self.lm(pre)
        self.prefix_of.update(new)
        self.calls += 1
        self.rows.append(n)
        return out


# ---------------------------------------------------------------------------------------------------- decoder case tables
# narrow beams against the reference decoder: (seed, T, C, width); the seeds were chosen so that every case's own smallest gap
# (fused_prefix_beam_search) exceeds NARROW_GAP -- test_cpu_lm_fusion.py asserts it for each, none is skipped
NARROW_GAP = 1e-4
NARROW_CASES = ((0, 20, 3, 3), (1, 33, 4, 3), (2, 47, 5, 8), (3, 60, 6, 8), (12, 28, 3, 8), (5, 52, 6, 3), (6, 41, 4, 8), (7, 24, 5, 3))
NARROW_LM_WEIGHT, NARROW_BONUS = 0.8, 0.3


def narrow_case(seed, T, C):
    rng = np.random.RandomState(100 + seed)
    return (rng.randn(T, C) * (0.5 if seed % 2 else 2.0)).astype(np.float32)


# the GPU decoder test: (seed, width) on posteriors of T 30, C 6 with a random LM; chosen with the float64 step on the CPU so that
# the reference's gap exceeds GPU_GAP
GPU_GAP = 1e-3
GPU_T, GPU_C, GPU_LENGTHS = 30, 6, (30, 17, 0)
GPU_LM_SHAPES = ((1, 16), (2, 48))                 # (L, H), V = 6
GPU_LM_WEIGHT, GPU_BONUS = 0.9, 0.2
GPU_CASES = {(1, 16): ((3, 4), (1, 8)), (2, 48): ((2, 4), (3, 8))}      # (L, H) -> ((seed, width), ..)


def gpu_posteriors(seed):
    rng = np.random.RandomState(500 + seed)
    return (rng.randn(GPU_T, len(GPU_LENGTHS), GPU_C) * 1.5).astype(np.float32)


def gpu_lm_params(L, H, seed=3):
    """A small random LM with enough contrast to move the beam: oracle.model's initialisation scaled up."""
    p = step_params(L, H, GPU_C, seed)
    p["output_w"] = (p["output_w"] * 3.0).astype(np.float32)
    p["input_w"] = (p["input_w"] * 2.0).astype(np.float32)
    return p


class OracleLm(object):
    """lm(prefix) through the float64 step, prefix by prefix from the zero state (cached): what LmStepper must reproduce."""

    def __init__(self, p, L):
        self.p, self.L = {k: v.astype(np.float64) for k, v in p.items()}, L
        self.V, self.H = p["input_w"].shape
        z = np.zeros((1, L, self.H))
        h, c, q = lm_step_ref(self.p, L, z, z, [self.V - 1])
        self.cache = {(): (h, c, q[0])}

    def __call__(self, prefix):
        prefix = tuple(prefix)
        if prefix not in self.cache:
            self(prefix[:-1])
            h, c, _ = self.cache[prefix[:-1]]
            h2, c2, q = lm_step_ref(self.p, self.L, h, c, [prefix[-1]])
            self.cache[prefix] = (h2, c2, q[0])
        return self.cache[prefix][2]
