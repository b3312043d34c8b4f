"""TEST INFRASTRUCTURE: the library-call sequence of one engine step, as data.

record(name) runs one configuration of CONFIGS with every public function of rnn_speech_amd.ops, torch.cuda.Stream.wait_event and
wait_stream replaced by pass-through wrappers (the real call still runs) and returns one entry per call, in call order:
[function name, argument, ...], the arguments in the order of the function's signature with its defaults filled in, so that a value
handed over by position, by keyword or left at its default reads the same.  An argument is recorded as
  a scalar or None                          itself
  a tensor                                  ["t", dtype, shape, strides, buffer label, element offset]: the label is the ordinal, by first
                                            appearance in this recording, of the base address of the tensor's storage -- which buffers
                                            alias, and where in them a view starts, is part of the record; raw addresses are not
  an object with a .buf (a workspace)       ["ws", class, descriptor fields (T, B, H, L, keep_in, keep_out, seed, precision) if it has a
                                            descriptor, its .buf as a tensor]
  a list or tuple                           the list of its members
  a CtcHead, a stream, an event             a fixed token
A call of after_lstm, beside_forward or beside_ctc is an entry of that name.  Calls that the library front makes to itself (a public ops
function from inside another) are the callee's business and are not entries.  tests/golden/engine_calls.json holds what the engine
recorded BEFORE it was rebuilt on the recurrence drivers (tools/make_golden.py --engine-calls); tests/test_gpu_engine_calls.py
requires every later engine to record exactly that.
"""
import contextlib
import functools
import inspect

import numpy as np

BASE = (2, 128, 20, 80, 3, 20, 8)          # (L, H, D, C, B, T, U): the smoke shape, lengths 20 / 13 / 17
BASE_LENGTHS = (20, 13, 17)

# name -> what the configuration runs.  shape / lengths / engine: the Engine's arguments and the batch; call: mini_batch's keywords;
# path: what kernel_path() has to say afterwards (a configuration that did not take the path it is named after fails); hooks: both side
# hooks given; fused: the module switch _FUSED_CTC for this run; run: "mini_batch" (default), "align", "lm_train", "lm_score".
# Where max_len = 17 is handed over the lengths are clamped to it: max_len is the host's knowledge of the longest row.
CONFIGS = {
    "uni_fused": dict(path=dict(fused_ctc_head=True, lstm_fwd="flow")),
    "uni_staged": dict(fused=False, path=dict(fused_ctc_head=False, lstm_fwd="flow")),
    "uni_fused_hooks": dict(hooks=True, path=dict(fused_ctc_head=True, lstm_fwd="flow")),
    "uni_staged_hooks": dict(fused=False, hooks=True, path=dict(fused_ctc_head=False, lstm_fwd="flow")),
    "uni_prefix_state_dropout": dict(lengths=(17, 13, 17), call=dict(max_len=17, use_state=True, keep_in=0.8, keep_out=0.5, seed=5),
                                     path=dict(run_length=17, lstm_fwd="flow")),
    "uni_eval": dict(call=dict(compute_gradients=False), path=dict(lstm_fwd="flow")),
    "uni_per_diagonal": dict(call=dict(per_diagonal=True), path=dict(fused_ctc_head=False, lstm_fwd="diag", lstm_bwd="diag")),
    "uni_norm": dict(engine=dict(normalization=True), path=dict(lstm_fwd="flow")),
    "uni_lookahead": dict(engine=dict(lookahead=3), path=dict(lookahead=3, fused_ctc_head=False)),
    "uni_conv": dict(engine=dict(conv=(16, 3, 3, 2, 2, 1)), path=dict(conv=16, run_length=10)),
    "uni_conv_lookahead_norm": dict(engine=dict(conv=(16, 3, 3, 2, 2, 1), lookahead=3, normalization=True),
                                    path=dict(conv=16, lookahead=3, fused_ctc_head=False)),
    "joined": dict(lengths=(17, 13, 17), engine=dict(bidirectional=True), call=dict(max_len=17), path=dict(paired=False, run_length=17)),
    "align": dict(run="align", path=dict(fused_ctc_head=False, run_length=20)),
    "uni_step": dict(shape=(2, 64, 20, 80, 5, 21, 8), lengths=(21, 9, 14, 1, 20), path=dict(lstm_fwd="diag", lstm_bwd="diag")),
    "joined_paired": dict(shape=(2, 1024, 40, 80, 64, 16, 6), engine=dict(bidirectional=True, precision="bf16"), path=dict(paired=True)),
    "layer_f32": dict(shape=(2, 64, 20, 30, 8, 30, 6), engine=dict(bidirectional=True, bidirectional_mode="layer"),
                      path=dict(layer_recurrence="persistent", layer_product="f32")),
    "layer_f32_per_diagonal": dict(shape=(2, 64, 20, 30, 8, 30, 6), engine=dict(bidirectional=True, bidirectional_mode="layer"),
                                   call=dict(per_diagonal=True), path=dict(layer_recurrence="per_frame", layer_product="f32")),
    "layer_bf16x3": dict(shape=(2, 64, 40, 80, 3, 17, 8), engine=dict(bidirectional=True, bidirectional_mode="layer", precision="bf16x3"),
                         path=dict(layer_recurrence="persistent", layer_product="bf16x3")),
    "lm_train": dict(run="lm_train", path=dict(run_length=9, lstm_fwd="flow")),
    "lm_score": dict(run="lm_score", path=dict(run_length=9, lstm_fwd="flow")),
}
LM_ENGINE = (2, 128, 30, 4, 12)             # LmEngine(L, H, V, B, T)


class Recorder(object):
    def __init__(self):
        self.entries, self._buffers, self._depth = [], {}, 0

    def _tensor(self, t):
        base = t.untyped_storage().data_ptr()
        label = self._buffers.setdefault(base, len(self._buffers))
        return ["t", str(t.dtype).replace("torch.", ""), list(t.shape), list(t.stride()), label, t.storage_offset()]

    def encode(self, v):
        import torch
        from rnn_speech_amd import ops
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if torch.is_tensor(v):
            return self._tensor(v)
        if isinstance(v, (list, tuple)):
            return [self.encode(m) for m in v]
        if isinstance(v, ops.CtcHead):
            return "CtcHead"
        if isinstance(v, torch.cuda.Stream):
            return "Stream"
        if isinstance(v, torch.cuda.Event):
            return "Event"
        if hasattr(v, "buf"):
            d = getattr(v, "desc", None)
            desc = None if d is None else [d.T, d.B, d.H, d.L, d.keep_in, d.keep_out, d.seed, d.precision]
            return ["ws", type(v).__name__, desc, self._tensor(v.buf)]
        raise TypeError("engine_calls: no encoding for an argument of type %s" % type(v).__name__)

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            if self._depth == 0:
                bound = sig.bind(*a, **kw)
                bound.apply_defaults()
                self.entries.append([name] + [self.encode(v) for v in bound.arguments.values()])
            self._depth += 1
            try:
                return fn(*a, **kw)
            finally:
                self._depth -= 1
        return wrapper

    def hook(self, name, fn):
        """A side hook of mini_batch (or forward's after_lstm) that enters itself before it runs."""
        def hooked(*a):
            self.entries.append([name] + [self.encode(v) for v in a])
            return fn(*a)
        return hooked

    @contextlib.contextmanager
    def recording(self):
        import torch
        from rnn_speech_amd import engine, ops
        saved = []

        def patch(owner, attr, new):
            saved.append((owner, attr, getattr(owner, attr)))
            setattr(owner, attr, new)

        for attr, fn in list(vars(ops).items()):
            if not attr.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
                patch(ops, attr, self.wrap(attr, fn))
        for attr in ("wait_event", "wait_stream"):
            patch(torch.cuda.Stream, attr, self.wrap("Stream." + attr, getattr(torch.cuda.Stream, attr)))
        forward = engine.Engine.forward
        fsig = inspect.signature(forward)

        def forward_with_named_hook(*a, **kw):
            bound = fsig.bind(*a, **kw)
            if bound.arguments.get("after_lstm") is not None:
                bound.arguments["after_lstm"] = self.hook("after_lstm", bound.arguments["after_lstm"])
            return forward(*bound.args, **bound.kwargs)
        patch(engine.Engine, "forward", forward_with_named_hook)
        try:
            yield self
        finally:
            for owner, attr, old in reversed(saved):
                setattr(owner, attr, old)


def dump(recorded, path):
    """{name: entries} as the golden file is kept: one line per entry."""
    import json
    blocks = ['"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries))
              for name, entries in recorded.items()]
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(blocks) + "\n}\n")


def _batch(L, H, D, C, B, T, U, lengths, conv):
    """Seeded features [T,B,D], the lengths and dense labels short enough for every row (over the model frames with the convolution)."""
    import torch
    rng = np.random.RandomState(H + B + T)
    x = rng.randn(T, B, D).astype(np.float32)
    lengths = np.asarray(lengths, np.int32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        frames = -(-int(lengths[b]) // conv[3]) if conv else int(lengths[b])
        n = max(0, min(U - 1, frames // 3))
        dense[b, :n] = 1 + (np.arange(n) * 7 + b) % (C - 2)
        dense[b, n] = C - 1
    return tuple(torch.as_tensor(a).cuda() for a in (x, lengths, dense))


def _assert_path(name, got, want):
    for k, v in want.items():
        assert got.get(k) == v, "%s did not take the path it is named after: %s is %r, not %r (%r)" % (name, k, got.get(k), v, got)


def record(name):
    """Run configuration `name` on the GPU under the recorder: its entries (JSON-ready lists)."""
    import torch
    from rnn_speech_amd import engine
    from rnn_speech_amd.language_model import LmEngine
    cfg = CONFIGS[name]
    rec = Recorder()
    run = cfg.get("run", "mini_batch")
    if run.startswith("lm_"):
        L, H, V, B, T = LM_ENGINE
        eng = LmEngine(L, H, V, B, T, seed=11)
        rng = np.random.RandomState(3)
        lens = np.array([9, 4, 7, 1], np.int32)
        tok = np.full((B, T + 1), V - 1, np.int32)
        for b in range(B):
            tok[b, 1:lens[b]] = rng.randint(0, V - 1, size=lens[b] - 1)
        tok, lens = torch.as_tensor(tok).cuda(), torch.as_tensor(lens).cuda()
        with rec.recording():
            if run == "lm_train":
                eng.zero_grads()
                eng.mini_batch(tok, lens, keep_in=0.9, keep_out=0.8, seed=4, max_len=9, scale=0.5)
                torch.cuda.synchronize()
                eng.check()
            else:
                eng.score(tok, lens, max_len=9)
        _assert_path(name, eng.kernel_path(), cfg["path"])
        return rec.entries
    shape = cfg.get("shape", BASE)
    L, H, D, C, B, T, U = shape
    lengths = cfg.get("lengths", BASE_LENGTHS if shape == BASE else [T - (5 * b) % (T // 2) for b in range(B)])
    kw = dict(cfg.get("engine", {}))
    eng = engine.Engine(L, H, D, C, B, T, U, seed=11, **kw)
    x, dlen, dense = _batch(L, H, D, C, B, T, U, lengths, kw.get("conv"))
    call = dict(cfg.get("call", {}))
    if cfg.get("hooks"):
        side = torch.cuda.Stream()

        def with_event(after):            # side work ordered behind `after` on a stream of its own: hands back its completion
            side.wait_event(after)
            done = torch.cuda.Event()
            done.record(side)
            return done
        call["beside_forward"] = rec.hook("beside_forward", with_event)
        call["beside_ctc"] = rec.hook("beside_ctc", lambda after: None)
    fused, engine._FUSED_CTC = engine._FUSED_CTC, cfg.get("fused", True)
    try:
        with rec.recording():
            if run == "align":
                eng.align(x, dlen, dense)
            else:
                eng.zero_grads()
                eng.mini_batch(x, dlen, dense, **call)
            torch.cuda.synchronize()
            eng.check()
    finally:
        engine._FUSED_CTC = fused
    _assert_path(name, eng.kernel_path(), cfg["path"])
    return rec.entries
