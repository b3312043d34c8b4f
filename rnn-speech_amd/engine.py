"""Device-side training engine for the acoustic model: flat parameter / gradient /
Adam buffers in HBM, the LSTM + CTC workspaces, and the op sequence of one
mini-batch and one optimiser step.  Everything numeric is a libamdspeech call
(ops.py); torch provides memory, streams and (for data parallel) the RCCL
all-reduce.

Mirrors what one `session.run` does in the reference:
  mini-batch  = models/AcousticModel.py:634-660  (forward, CTC, gradients += )
  apply       = models/AcousticModel.py:672-703  (clip_by_global_norm + Adam)
"""
import contextlib
import math
import os

import numpy as np
import torch

from . import lib as _lib
from . import ops
from . import stacks


def _pad64(n):
    return (n + 63) // 64 * 64


class ParamLayout(object):
    """Flat fp32 layout [input_w | input_b | (kernel_l | bias_l)*L | output_w | output_b | lookahead_w (lookahead > 0 only) |
    conv_w | conv_b (conv only)], every tensor starting on a 256-byte boundary (pads are zero and stay zero).  `input_dim` is the
    width the input Linear reads: with `conv` = (C, kt, kf, st, sf, G) that is F' * C, the convolution's output."""

    def __init__(self, num_layers, hidden, input_dim, num_labels, bidirectional=False, bidirectional_mode="top", lookahead=0, conv=None):
        self.L, self.H, self.D, self.C = num_layers, hidden, input_dim, num_labels
        self.bidirectional = bool(bidirectional)
        self.lookahead = int(lookahead)
        self.conv = tuple(int(v) for v in conv) if conv else None
        # "layer" (stack_bidirectional_dynamic_rnn): the cells above layer 0 read [h_fw ; h_bw], kernels (3H, 4H) there -- the stride
        # between layers is not uniform (kernel_stride / bias_stride are None)
        self.layerwise = self.bidirectional and bidirectional_mode == "layer"
        off = 0
        self.slots = {}

        def take(name, shape):
            nonlocal off
            n = 1
            for s in shape:
                n *= s
            self.slots[name] = (off, shape)
            off += _pad64(n)

        take("input_w", (input_dim, hidden))
        take("input_b", (hidden,))
        def rows(l):
            return (3 if self.layerwise and l > 0 else 2) * hidden

        for l in range(num_layers):
            take("kernel_%d" % l, (rows(l), 4 * hidden))
            take("bias_%d" % l, (4 * hidden,))
        if self.bidirectional:           # the backward-direction stack: same shapes, same stride between layers
            for l in range(num_layers):
                take("bw_kernel_%d" % l, (rows(l), 4 * hidden))
                take("bw_bias_%d" % l, (4 * hidden,))
        take("output_w", ((2 if self.bidirectional else 1) * hidden, num_labels))
        take("output_b", (num_labels,))
        if self.lookahead > 0:           # the row convolution's taps: LAST, so that no other tensor moves when the option is on
            take("lookahead_w", (self.lookahead + 1, hidden))
        if self.conv:                    # the front convolution's filter bank and bias: behind everything else, for the same reason
            c, kt, kf, _, _, g = self.conv
            take("conv_w", (g * kt * kf, c))
            take("conv_b", (c,))
        self.total = off
        if self.layerwise:
            self.kernel_stride = self.bias_stride = None
        elif num_layers > 1:
            self.kernel_stride = self.slots["kernel_1"][0] - self.slots["kernel_0"][0]
            self.bias_stride = self.slots["bias_1"][0] - self.slots["bias_0"][0]
        else:
            self.kernel_stride = self.bias_stride = 0

    def names(self):
        return list(self.slots.keys())

    def view(self, flat, name):
        off, shape = self.slots[name]
        n = 1
        for s in shape:
            n *= s
        return flat[off:off + n].view(*shape)

    def num_params(self):
        tot = 0
        for _, shape in self.slots.values():
            n = 1
            for s in shape:
                n *= s
            tot += n
        return tot


_BESIDE_FORWARD = os.environ.get("AMDSPEECH_BESIDE_FORWARD", "1") != "0"      # 0: the side work always goes beside the CTC stage
_BESIDE_TAIL = os.environ.get("AMDSPEECH_BESIDE_TAIL", "1") != "0"            # 0: the dense layers' weight gradients behind the LSTM's
_BIDIR_PAIR = os.environ.get("AMDSPEECH_BIDIR_PAIR", "1") != "0"              # 0: a bidirectional model's two stacks as two lstm_fwd calls
_FUSED_CTC = os.environ.get("AMDSPEECH_FUSED_CTC", "1") != "0"                # 0: the CTC stage as launches between the two recurrence kernels


# amdspeech_lstm_desc.precision of the stacked-LSTM products (recurrent AND batched): exact f32 MFMA (what the reference computes,
# the default and the headline), bf16 hi/lo pairs (three MFMAs per product, ~16 significant bits), plain bf16 (one MFMA, 8 bits:
# BASELINE configs[4]'s "bf16 MFMA").  Gates, cell state, gradients, accumulation, master weights and Adam are f32 in every mode.
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}


class ParamStore(object):
    """Everything that hangs off a ParamLayout and a device, for every model: the flat fp32 parameter / gradient / Adam buffers,
    views and host copies by tensor name, Glorot initialisation, the optimiser step, and the health predicate and run-length clamp
    of the engines built on it.  A subclass sets T (its padded length) and B, H, its logits / dlogits buffers and its recurrence
    driver `stack` (stacks.py), and says what it is in _describe()."""

    def __init__(self, layout, device, storage=None):
        """storage: the four flat buffers (params, grads, adam_m, adam_v) of layout.total floats each, for a store that is a part
        of a larger one (transducer.TransducerEngine: one clip and one Adam over every part); None allocates them."""
        self.layout, self.device = layout, torch.device(device)
        if storage is None:
            storage = tuple(torch.zeros(layout.total, device=self.device) for _ in range(4))
        if len(storage) != 4 or any(t.numel() != layout.total or not t.is_contiguous() for t in storage):
            raise ValueError("storage must be four contiguous flat buffers of %d floats" % layout.total)
        self.params, self.grads, self.adam_m, self.adam_v = storage
        self.norm = torch.zeros(1, device=self.device)
        self.adam_step = 0

    def p(self, name):
        return self.layout.view(self.params, name)

    def g(self, name):
        return self.layout.view(self.grads, name)

    def init_parameters(self, seed=1234):
        """Xavier/Glorot-uniform matrices, zero biases (TF defaults, :241-244,302-305).  The lookahead taps start as the identity
        (w[0] = 1, the future taps 0) and draw nothing: every other tensor has the values it has without them.  The front
        convolution's filters are Glorot-uniform over their receptive fields: fan-in K = G kt kf, fan-out kt kf C."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        self.params.zero_()
        for name in self.layout.names():
            _, shape = self.layout.slots[name]
            if name == "lookahead_w":
                self.p(name)[0].fill_(1.0)
            elif len(shape) == 2:
                lim = math.sqrt(6.0 / (shape[0] + shape[1]))
                if name == "conv_w":
                    c, kt, kf = self.layout.conv[:3]
                    lim = math.sqrt(6.0 / (shape[0] + kt * kf * c))
                w = (torch.rand(shape, generator=gen) * 2.0 - 1.0) * lim
                self.p(name).copy_(w)

    def load_numpy(self, arrays, flat=None):
        """Copy host arrays into the flat buffer (default: the parameters).  Shapes must match the layout exactly:
        copy_ would silently broadcast e.g. a shape-(1,) bias from a checkpoint of another model size."""
        flat = self.params if flat is None else flat
        for name, a in arrays.items():
            if name not in self.layout.slots:
                raise KeyError("unknown parameter tensor %r (layout has %s)" % (name, ", ".join(self.layout.names())))
            want = tuple(self.layout.slots[name][1])
            got = tuple(np.shape(a))
            if got != want:
                raise ValueError("checkpoint tensor %s has shape %s, %s needs %s" % (name, got, self._describe(), want))
            self.layout.view(flat, name).copy_(torch.as_tensor(np.asarray(a), dtype=torch.float32))

    def to_numpy(self, flat=None):
        flat = self.params if flat is None else flat
        return {n: self.layout.view(flat, n).detach().cpu().numpy().copy() for n in self.layout.names()}

    def zero_grads(self):
        self.grads.zero_()

    def apply(self, lr, clip, beta1=0.9, beta2=0.999, eps=1e-8):
        self.adam_step += 1
        t = self.adam_step
        lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        ops.clip_adam(self.params, self.grads, self.adam_m, self.adam_v, float(clip), lr_t, beta1, beta2, eps,
                      norm_out=self.norm)
        return self.norm

    def healthy(self):
        """check() as a predicate: False when a dataflow launch of the last mini-batch gave up waiting (its results -- logits, loss,
        the gradient contribution, the final state -- are invalid; see mini_batch(per_diagonal=True) for the way out).  Only the
        time-out is recoverable: any other error of the status call (a sticky HIP fault) is raised, not turned into a retry."""
        try:
            self.check()
            return True
        except _lib.DataflowTimeout:
            return False

    # ---- what the engines built on the store share: the recurrence driver `stack` (stacks.py), logits / dlogits [T,B,C] --------
    _ws = property(lambda self: self.stack.ws)                # the stack's (forward-direction) workspace at the last run length
    lstm_ws = property(lambda self: self.stack.lstm_ws)       # ... and its allocation

    def check(self):
        """Synchronous health check of the dataflow LSTM kernels: their waits are bounded, and a time-out (the
        workgroups of one launch were not all resident -- another kernel held CUs) leaves an error flag behind
        instead of hanging.  Raises AmdSpeechError; results of that step are invalid."""
        self.stack.check()

    def _output_fwd(self, tops, Tr):
        """The output layer over the one or two top outputs [(y, dy), ..]: logits[:Tr] = [y_0 ; y_1] . W_o + b_o."""
        n, H, wo = Tr * self.B, self.H, self.p("output_w")
        out = self.logits[:Tr].view(n, -1)
        ops.linear_fwd(tops[0][0].view(n, H), wo[:H], self.p("output_b"), out=out)
        for y, _ in tops[1:]:
            ops.gemm(y.view(n, H), wo[H:], out=out, accumulate=True)

    def _fill_tail(self, Tr):
        """Rows past the run length are the output bias (what the reference produces there: the LSTM output is zero past the length)."""
        if Tr < self.T:
            self.logits[Tr:] = self.p("output_b")          # broadcast fill of the never-visited tail

    def _output_bwd(self, tops, Tr, need_dx=True):
        """dW_o += [y_0 ; y_1]^T . dlogits, db_o += column sums of dlogits and (need_dx) dy_i = dlogits . W_o[half i]^T."""
        n, H = Tr * self.B, self.H
        wo, gwo, dl = self.p("output_w"), self.g("output_w"), self.dlogits[:Tr].view(n, -1)
        y, dy = tops[0]
        ops.linear_bwd(y.view(n, H), wo[:H], dl, gwo[:H], self.g("output_b"), need_dx=need_dx, dx=dy.view(n, H) if need_dx else None)
        for y, dy in tops[1:]:
            ops.gemm(y.view(n, H), dl, trans_a=True, out=gwo[H:], accumulate=True)
            ops.gemm(dl, wo[H:], trans_b=True, out=dy.view(n, H))

    def _run_length(self, max_len):
        """Steps the recurrence has to visit: the longest row of this batch when the host knows it (`max_len`, from the dataset
        pipeline -- no device sync), else the padded length.  Mirrors tf.nn.dynamic_rnn, whose while-loop runs to
        max(sequence_length) (reference :276-278)."""
        return self.T if max_len is None else max(1, min(int(max_len), self.T))


class Engine(ParamStore):
    def __init__(self, num_layers, hidden, input_dim, num_labels, batch_size, max_T, max_U,
                 device="cuda", seed=1234, normalization=False, precision="f32", bidirectional=False,
                 sync_batch_norm=False, bidirectional_mode="top", lookahead=0, conv=None, storage=None):
        if not torch.cuda.is_available():
            raise RuntimeError("rnn_speech_amd needs a ROCm GPU (MI355X); there is no CPU path")
        # strided time-frequency convolution between the features and the input Linear (ops.conv2d_fwd; no reference counterpart,
        # off at None: nothing of it is allocated or launched).  conv = (C, kt, kf, st, sf, G).  The caller hands SOURCE frames
        # [T_in, B, D_in = G * F] and source lengths; everything from the input Linear on sees T = ceil(T_in / st) model frames of
        # D = ceil(F / sf) * C values and the model lengths the convolution's launch writes (model_lengths)
        self.conv = tuple(int(v) for v in conv) if conv else None
        self.T_in, self.D_in = max_T, input_dim
        if self.conv:
            c, kt, kf, st, sf, g = self.conv
            if g < 1 or input_dim % g:
                raise ValueError("conv: %d feature groups do not divide the %d values of a source frame" % (g, input_dim))
            ops.conv2d_check(c, kt, kf, st, sf, F=input_dim // g)
            max_T, input_dim = ops.conv2d_out_shape(max_T, input_dim // g, c, st, sf)
        self.L, self.H, self.D, self.C = num_layers, hidden, input_dim, num_labels
        self.B, self.T, self.U = batch_size, max_T, max_U
        # bidirectional (BASELINE configs[4]; no reference counterpart -- the reference builds a unidirectional dynamic_rnn,
        # :276-278): a second stack of the same shape reads every utterance reversed in time (tf.reverse_sequence semantics,
        # as tf.nn.bidirectional_dynamic_rnn does), the two top outputs are concatenated in front of the output layer
        self.bidirectional = bool(bidirectional)
        if bidirectional_mode not in ("top", "layer"):
            raise ValueError("bidirectional_mode must be 'top' (two stacks joined in front of the output layer) or 'layer' "
                             "(stack_bidirectional_dynamic_rnn: every layer reads both directions of the layer below)")
        # layer-wise bidirectional stacks (amdspeech_lstm_bidir_*): only read when bidirectional
        self.layerwise = self.bidirectional and bidirectional_mode == "layer"
        if self.layerwise and precision not in ("f32", "bf16x3"):
            raise ValueError("bidirectional_mode 'layer' runs in exact f32 or bf16x3 (precision %r requested): the layer-wise kernels "
                             "have no plain-bf16 variant" % (precision,))
        # lookahead (row) convolution between the top layer and the output layer (ops.lookahead_fwd; no reference counterpart, off at
        # 0: nothing of it is allocated or launched): `lookahead` future frames of context for a model that stays unidirectional
        self.lookahead = int(lookahead)
        if not 0 <= self.lookahead <= ops.LOOKAHEAD_MAX_CONTEXT:
            raise ValueError("lookahead must be 0 (off) .. %d future frames, not %r" % (ops.LOOKAHEAD_MAX_CONTEXT, lookahead))
        if self.lookahead and self.bidirectional:
            raise ValueError("lookahead %d with a bidirectional model: the row convolution gives a UNIDIRECTIONAL stack its future "
                             "context; a bidirectional stack already reads the whole utterance" % self.lookahead)
        ParamStore.__init__(self, ParamLayout(num_layers, hidden, input_dim, num_labels, bidirectional=self.bidirectional,
                                              bidirectional_mode="layer" if self.layerwise else "top", lookahead=self.lookahead,
                                              conv=self.conv), device, storage)
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'f32' (exact, default), 'bf16x3' (split-precision MFMA) or 'bf16' (plain bf16 "
                             "operands, f32 accumulation and master weights)")
        self.precision = precision
        # the recurrence driver: the one place that knows which arrangement of stacks this engine runs
        driver = stacks.LayerStack if self.layerwise else stacks.JoinedStack if self.bidirectional else stacks.UniStack
        self.stack = driver(self, max_T, batch_size, hidden, num_layers, PRECISIONS[precision])
        if self.lookahead:               # f32 in every precision mode
            self.la_y = torch.empty(max_T, batch_size, hidden, device=self.device)        # the convolution's output: what the output layer reads
            self.la_dy = torch.empty(max_T, batch_size, hidden, device=self.device)
            self.la_ws = ops.LookaheadWorkspace(max_T, batch_size, hidden, self.lookahead, device=self.device)
        if self.conv:                    # f32 in every precision mode
            c, kt, kf, st, sf, g = self.conv
            self.cv_y = torch.empty(max_T, batch_size, input_dim, device=self.device)     # the convolution's output: what the input Linear reads
            self.cv_dy = torch.empty(max_T, batch_size, input_dim, device=self.device)
            self.cv_len = torch.zeros(batch_size, device=self.device, dtype=torch.int32)  # model lengths of the last forward
            self.cv_ws = ops.Conv2dWorkspace(self.T_in, batch_size, g, self.D_in // g, c, kt, kf, st, sf, device=self.device)
        self.ctc_ws = ops.CtcWorkspace(max_T, batch_size, num_labels, max_U, self.device)
        self.logits = torch.empty(max_T, batch_size, num_labels, device=self.device)
        self.dlogits = torch.empty_like(self.logits)
        self.loss = torch.zeros(batch_size, device=self.device)
        # persistent RNN state Variables of the reference (:266-275)
        self.state_h = torch.zeros(num_layers, batch_size, hidden, device=self.device)
        self.state_c = torch.zeros(num_layers, batch_size, hidden, device=self.device)
        # optional batch norm of the input-layer output (reference :253-259, off by default)
        self.normalization = bool(normalization)
        # Under data parallelism the moments are taken over THIS rank's mini-batch by default: N ranks x batch b is the
        # reference's mini_batch_size = N accumulation, and the reference normalises every mini-batch with its own moments
        # (:253-259 inside the per-mini-batch graph).  sync_batch_norm=True (opt-in, a DEVIATION from the reference: a
        # different model, three blocking all-reduces per mini-batch, no early stop at the longest utterance) spans the ranks.
        self.sync_batch_norm = bool(sync_batch_norm) and self.normalization
        if self.normalization:
            self.bn_xhat = torch.empty(max_T, batch_size, hidden, device=self.device)
            self.bn_inv_std = torch.empty(max_T, hidden, device=self.device)
            self.bn_scratch = torch.empty(2, max_T, hidden, device=self.device)       # cross-rank sums under data parallelism
        self._Tr = max_T                 # frames the last forward visited
        self._head = None                # ops.CtcHead of the mini-batch in flight, when its CTC stage runs inside the LSTM launches
        self._tops = self._la_x = None   # (y, dy) pairs of the last forward: what the output layer read, what the lookahead read
        # a real (non-NULL) stream for callers that want the overlapped backward pass: see on_stream()
        self.stream = torch.cuda.Stream(device=self.device, priority=-1)      # (ahead of the side stream that prefetches the next batch)
        self._aux_stream = None          # (mini_batch: carries the "beside the forward kernel" ordering point to the caller's hook)
        self.init_parameters(seed)

    # (names that tests of the two bidirectional arrangements read: the backward-direction stack's workspace, the 2L cell tensors)
    _ws_b = property(lambda self: self.stack.bw.ws)
    _cells = property(lambda self: self.stack.cells)

    def _describe(self):
        return "the model (L=%d, H=%d, D=%d, C=%d)" % (self.L, self.H, self.D, self.C)

    @staticmethod
    def _dp_group():
        from . import dataparallel
        return dataparallel.current()

    # ---- one mini-batch ----------------------------------------------------------
    def _run_length(self, max_len):
        """Frames the recurrence has to visit: ParamStore's clamp to the longest utterance, with one exception."""
        if max_len is not None and self.sync_batch_norm and self._dp_group().world > 1:
            return self.T          # the batch moments span the ranks: every rank contributes all T frames (padding included)
        return ParamStore._run_length(self, max_len)

    def forward(self, x, lengths, keep_in=1.0, keep_out=1.0, seed=0, use_state=False, max_len=None, after_lstm=None, training=False,
                per_diagonal=False, dense_labels=None):
        """x [T,B,D] device float32, lengths int32 [B] device.  Returns logits [T,B,C]
        (a view of the engine's buffer).  Rows past `max_len` are the output bias (what the
        reference produces there, since the LSTM output is zero past the length).
        With the front convolution x is [T_in,B,D_in], lengths and max_len count SOURCE frames, and the logits are the T model
        frames; model_lengths() has the rows' lengths in model frames."""
        T, B, D = x.shape
        assert (T, B, D) == (self.T_in, self.B, self.D_in), ((T, B, D), (self.T_in, self.B, self.D_in))
        D, H = self.D, self.H
        x = x.contiguous()
        if self.conv and max_len is not None:
            max_len = -(-max(int(max_len), 0) // self.conv[3])       # the run length is counted in model frames
        Tr = self._Tr = self._run_length(max_len)
        stack = self.stack
        stack.lay_out(Tr, keep_in, keep_out, seed)
        z0 = stack.z0
        # 1. front convolution
        if self.conv:
            c, kt, kf, st, sf, g = self.conv
            ops.conv2d_fwd(x[:self._source_run(Tr)], self.p("conv_w"), self.p("conv_b"), lengths, g, (kt, kf), (st, sf),
                           out=self.cv_y[:Tr], lengths_out=self.cv_len)
            x, lengths = self.cv_y, self.cv_len          # from here on: model frames, model lengths
        # 2. input Linear
        ops.linear_fwd(x[:Tr].view(Tr * B, D), self.p("input_w"), self.p("input_b"), out=z0.view(Tr * B, H))
        # 3. batch norm
        if self.normalization:
            self._batchnorm_fwd(z0, Tr)
        # 4. recurrence.  With the CTC head inside the LSTM launches (ops.CtcHead; dense_labels given = a training mini-batch) the
        # output layer, the log-softmax and alpha follow the forward recurrence, beta and the gradient lead the backward one
        self._head = None
        if (dense_labels is not None and _FUSED_CTC and not self.lookahead
                and stack.ctc_fusable(self.C, dense_labels.shape[1], per_diagonal)):
            self._head = ops.CtcHead(self.p("output_w"), self.p("output_b"), self.logits[:Tr], dense_labels, self.loss,
                                     self.dlogits[:Tr], self.ctc_ws)
        stack.forward(lengths, self.state_h if use_state else None, self.state_c if use_state else None, training, per_diagonal,
                      self._head, pair=_BIDIR_PAIR)
        # 5. the caller's hook
        if after_lstm is not None:
            after_lstm()           # (mini_batch: from here on other streams may use the chip -- see beside_ctc)
        # 6. lookahead (the fused head is never taken with it: the output layer reads the convolution's output)
        self._tops = stack.tops(lengths)
        if self.lookahead:
            self._la_x = self._tops[0]
            ops.lookahead_fwd(self._la_x[0], self.p("lookahead_w"), lengths, out=self.la_y[:Tr])
            self._tops = [(self.la_y[:Tr], self.la_dy[:Tr])]
        # 7. output layer
        if self._head is None:
            self._output_fwd(self._tops, Tr)
        # 8. tail fill
        self._fill_tail(Tr)
        return self.logits

    def _batchnorm_fwd(self, z0, Tr):
        grp = self._dp_group() if self.sync_batch_norm else None
        if grp is not None and grp.world > 1:      # moments over the GLOBAL batch: local sums -> all-reduce -> finish (Tr == T on every rank)
            ops.batchnorm_fwd_dp(z0, z0, self.bn_xhat, self.bn_inv_std, grp, self.bn_scratch, 1e-3)
        else:
            ops.batchnorm_fwd(z0, z0, self.bn_xhat[:Tr], self.bn_inv_std[:Tr], 1e-3)

    def _batchnorm_bwd(self, dz0, Tr):
        grp = self._dp_group() if self.sync_batch_norm else None
        if grp is not None and grp.world > 1:
            ops.batchnorm_bwd_dp(dz0, self.bn_xhat, self.bn_inv_std, dz0, grp, self.bn_scratch)
        else:
            ops.batchnorm_bwd(dz0, self.bn_xhat[:Tr], self.bn_inv_std[:Tr], dz0)

    def _source_run(self, Tr):
        """Source frames behind a run of Tr model frames (ceil(that / st) == Tr)."""
        return min(self.T_in, Tr * self.conv[3])

    def model_lengths(self, lengths):
        """The rows' lengths as everything behind the input Linear counts them: the device tensor the front convolution's launch of
        the LAST forward wrote (ceil(min(length, run) / st)), or `lengths` itself without that layer."""
        return self.cv_len if getattr(self, "conv", None) else lengths      # (getattr: engines that stand in for this one in tests)

    def _input_linear_bwd(self, x, lengths, Tr):
        """The input Linear's weight gradients from dZ_0; with the front convolution also dZ_0 . W_i^T into its dy buffer and the
        convolution's own gradients (x and lengths are the SOURCE ones), queued on the current stream."""
        n = Tr * self.B
        x_in, dx = (self.cv_y, self.cv_dy[:Tr].view(n, self.D)) if self.conv else (x, None)
        ops.linear_bwd(x_in[:Tr].view(n, self.D), self.p("input_w"), self.stack.dz0.view(n, self.H), self.g("input_w"), self.g("input_b"),
                       need_dx=dx is not None, dx=dx)
        if self.conv:
            c, kt, kf, st, sf, g = self.conv
            ops.conv2d_bwd(x[:self._source_run(Tr)], self.cv_y[:Tr], self.cv_dy[:Tr], lengths, g, (kt, kf), (st, sf),
                           self.g("conv_w"), self.g("conv_b"), ws=self.cv_ws)

    def kernel_path(self):
        """Which shape-driven choices the LAST forward made -- what a parity test has to assert before it may claim to have checked
        them: `fused_ctc_head` (the CTC stage ran inside the two whole-sequence LSTM launches, ops.CtcHead), `paired` (a
        bidirectional model's two stacks side by side on one-XCD groups, ops.lstm_fwd_pair), `run_length` (frames visited), and
        `lookahead` (the row convolution's context, 0 = none: with it the fused head is never taken), `conv` (the front
        convolution's channels, 0 = none: with it `run_length` counts model frames of its output), `lstm_fwd` / `lstm_bwd`: the
        kernel path of that forward and of the backward that belongs to it ("flow", "big1", "big", "hoist", "diag", "diag_bf3":
        ops.lstm_plan at the run length, with the head and the per-diagonal request of the call); a layer-wise stack names
        `layer_recurrence` and `layer_product` instead (stacks.LayerStack.kernel_path)."""
        path = {"fused_ctc_head": self._head is not None, "lookahead": self.lookahead, "paired": self.stack.paired,
                "run_length": self._Tr, "conv": self.conv[0] if self.conv else 0}
        path.update(self.stack.kernel_path(self._head))
        return path

    def final_state(self):
        """(h [L,B,H], c [L,B,H]) after the last forward."""
        return self._ws.final_state()

    def keep_state(self):
        """rnn_keep_state_op (:281-289): final state -> persistent state."""
        h, c = self._ws.final_state()
        self.state_h.copy_(h)
        self.state_c.copy_(c)

    def zero_state(self):
        self.state_h.zero_()
        self.state_c.zero_()

    def ctc(self, dense_labels, lengths, stage=0):
        Tr = self._Tr
        lengths = self.model_lengths(lengths)
        if self._head is None:           # (with the head the loss is the forward launch's; dlogits will be the backward launch's)
            ops.ctc_loss_fwd_bwd(self.logits[:Tr], dense_labels, lengths, ws=self.ctc_ws, loss=self.loss,
                                 dlogits=self.dlogits[:Tr], stage=stage)
        if Tr < self.T and stage != 1:   # the never-visited tail carries no gradient
            self.dlogits[Tr:].zero_()
        return self.loss

    def align(self, x, lengths, dense_labels):
        """Forced alignment of known transcripts: a forward pass in inference mode (no dropout) and the best CTC alignment of
        `dense_labels` (int32 [B,U], 0-padded as mini_batch takes them) to the frames of its logits.  Returns an ops.CtcAlignment
        (frame_label / frame_state [B,T], spans [B,U,2], score [B], confidence [B,U]).  Reads the logits only: every stack the
        engine builds (uni-directional, top-joined and layer-wise bidirectional) takes it."""
        self.forward(x, lengths)
        shape = (self.T, self.B, self.C, dense_labels.shape[1])
        if getattr(self, "_align_ws", None) is None or self._align_ws.shape != shape:
            self._align_ws = ops.CtcAlignWorkspace(*shape, device=self.device)
        return ops.ctc_align(self.logits, dense_labels.contiguous(), self.model_lengths(lengths), ws=self._align_ws)

    @contextlib.contextmanager
    def on_stream(self):
        """Run the enclosed engine calls on the engine's own (non-default) stream, ordered after the
        caller's current stream and joined back into it on exit.  The backward pass overlaps the weight-
        gradient GEMMs with the BPTT chain on CU-partitioned HIP streams; those are "blocking" streams, so
        the overlap is only used (and only pays off) when the work is NOT issued on the legacy NULL stream
        (csrc/lstm.hip, lstm_bwd).  A caller that already sits on a real stream is left there."""
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != 0:
            yield
            return
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield
        cur.wait_stream(self.stream)

    def backward(self, x, lengths, wait_for=None, per_diagonal=False):
        """Accumulates d(sum_b loss_b)/d(theta) into self.grads (for the batch of the last forward).
        wait_for: an event the backward RECURRENCE has to wait for (side-stream work placed beside the CTC stage)."""
        x = x.contiguous()
        stack, Tr = self.stack, self._Tr
        src_lengths, lengths = lengths, self.model_lengths(lengths)      # (the source lengths are the front convolution's alone)
        head = self._head
        if head is not None and per_diagonal:
            raise _lib.AmdSpeechError("backward(per_diagonal=True) after a forward with the fused CTC head: repeat the forward too")
        if head is None:                 # (with the head dlogits and dZ_top are formed inside the recurrence's launch; dW_o / db_o follow it)
            # 1. output layer
            self._output_bwd(self._tops, Tr)
            # 2. lookahead: the output layer read the convolution's output; its dx is the convolution's dy
            if self.lookahead:
                y, dy = self._la_x
                ops.lookahead_bwd(y, self.p("lookahead_w"), self.la_dy[:Tr], lengths, dx=dy, dw=self.g("lookahead_w"), ws=self.la_ws)
            stack.take_dtops(lengths)
        # 3. the side work the recurrence must not start beside
        if wait_for is not None:
            torch.cuda.current_stream(self.device).wait_event(wait_for)
        # 4. recurrence
        stack.backward(lengths, per_diagonal, head, pair=_BIDIR_PAIR)
        # 5. tail overlap: the dense layers' weight gradients beside the first of the weight-gradient launches that follow the
        # backward kernel (stacks.UniStack.beside_tail) instead of behind the last
        side, dz0_ready = stack.beside_tail() if _BESIDE_TAIL and not self.normalization and not per_diagonal else (None, False)
        if side is not None:
            with torch.cuda.stream(side):
                if head is not None:
                    self._output_bwd(self._tops, Tr, need_dx=False)
                if dz0_ready:            # (with the front convolution: its gradients too, queued before the join below)
                    self._input_linear_bwd(x, src_lengths, Tr)
            torch.cuda.current_stream(self.device).wait_stream(side)
        elif head is not None:
            self._output_bwd(self._tops, Tr, need_dx=False)
        # 6. batch norm
        if self.normalization:
            self._batchnorm_bwd(stack.dz0, Tr)
        # 7. input Linear and convolution
        if side is None or not dz0_ready:
            self._input_linear_bwd(x, src_lengths, Tr)

    def mini_batch(self, x, lengths, dense_labels, keep_in=1.0, keep_out=1.0, seed=0, use_state=False,
                   compute_gradients=True, max_len=None, beside_ctc=None, marks=None, beside_forward=None, per_diagonal=False):
        """forward -> CTC -> backward, with two slots for side work on other streams; each is an optional
        callable(after_event) -> done_event (or None) that enqueues short-lived kernels / copies ordered after `after_event`:
          beside_forward: work that needs NOTHING of this mini-batch (the next one's front end).  When the forward recurrence
            is the whole-sequence dataflow kernel with XCDs to spare, `after_event` is the point just in front of its launch
            (ops.lstm_beside_forward): the front end's work-queue kernel then does its work on the idle XCDs while the
            recurrence runs (and completes with it).  Otherwise the call comes in the other slot;
          beside_ctc: work that needs this mini-batch's LOGITS (the training-time decoder's copy): beside the CTC recursions
            between the two recurrence kernels (64 of the 256 CUs busy for ~0.2 ms).
        The backward recurrence waits for both.  Nothing is ever placed beside the backward kernel: it keeps every CU.
        per_diagonal: run the stack on the launch-per-diagonal kernels (amdspeech.h: AMDSPEECH_LSTM_PER_DIAGONAL) -- the repeat of
        a mini-batch whose whole-sequence launch timed out (healthy() is False); same results, no co-residency requirement."""
        def mark(name):                # (timeline: HIP events between the stages, read by the caller after a sync)
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(torch.cuda.current_stream(self.device))
                marks.append((name, ev))

        mark("begin")
        placed = []

        def try_beside_forward():
            # the XCDs the whole-sequence forward kernel leaves without a recurrence group (two of eight for ~5 ms at 3x512 /
            # batch 32): amdspeech_lstm_beside_forward.  Beside the CTC recursions the same work shares SIMDs with them
            # (alpha/beta 150 -> 250 us with the matrix-core front end next to it).
            if beside_forward is None or not _BESIDE_FORWARD:
                return
            if self._aux_stream is None:
                self._aux_stream = torch.cuda.Stream(self.device)
            if self.stack.beside_forward(self._aux_stream) > 0:
                after = torch.cuda.Event()
                after.record(self._aux_stream)
                placed.append(beside_forward(after))

        self.forward(x, lengths, keep_in, keep_out, seed, use_state, max_len, training=compute_gradients, after_lstm=try_beside_forward,
                     per_diagonal=per_diagonal, dense_labels=dense_labels)
        mark("forward")
        pending = [ev for ev in placed if ev is not None]
        late = [h for h in (beside_ctc, (beside_forward if not placed else None)) if h is not None]

        def place_late():              # the late hooks, ordered behind what the current stream holds now
            after = torch.cuda.Event()
            after.record(torch.cuda.current_stream(self.device))
            for h in late:
                ev = h(after)
                if ev is not None:
                    pending.append(ev)

        fused = self._head is not None
        if fused:
            # The CTC stage ran inside the forward launch and will finish inside the backward one: there is no stage to place work
            # beside.  Hooks that need the logits are ordered behind the forward launch and JOINED BEHIND the backward pass: short
            # kernels and copies that become runnable together with the backward kernel either slip in front of it (the library's
            # own side-stream fills keep that launch waiting ~0.1 ms anyway) or run when it ends -- they depend on nothing of it,
            # so its workgroups never wait for more than their duration.
            place_late()
            self.ctc(dense_labels, lengths)
        elif late:
            # behind the output layer and the log-softmax (both fill the chip and are short), beside the CTC recursions
            self.ctc(dense_labels, lengths, stage=1)
            place_late()
            self.ctc(dense_labels, lengths, stage=2)
        else:
            self.ctc(dense_labels, lengths)
        mark("ctc")
        cur = torch.cuda.current_stream(self.device)
        # the side work is joined in front of the backward RECURRENCE (its last event inside backward(), behind the output layer's
        # gradients) -- or, with the fused head, behind the whole backward pass
        ahead = [] if fused else pending
        for ev in ahead[:-1]:
            cur.wait_event(ev)
        done = ahead[-1] if ahead else None
        if compute_gradients:
            self.backward(x, lengths, wait_for=done, per_diagonal=per_diagonal)
            mark("backward")
        elif done is not None:
            cur.wait_event(done)      # the next recurrence kernel must not start beside it
        if fused:
            for ev in pending:
                cur.wait_event(ev)
        return self.loss

    # ---- data parallel (the optimiser step itself is ParamStore.apply) ----------------
    def all_reduce_grads(self):
        """Data parallel: ONE fused fp32 SUM all-reduce of the flat gradient buffer (amdspeech_allreduce_sum_f32 =
        RCCL over xGMI, see dataparallel.py); N ranks x batch b is then the reference's mini_batch_size=N
        accumulation (:391-406).  A no-op in a single-process job."""
        from . import dataparallel
        dataparallel.current().all_reduce_sum_(self.grads)

    def broadcast_state(self, root=0):
        """Make every replica bit-identical to rank `root`: parameters and Adam moments (after a restore)."""
        from . import dataparallel
        grp = dataparallel.current()
        for flat in (self.params, self.adam_m, self.adam_v):
            grp.broadcast_(flat, root)
        self.adam_step = int(grp.broadcast_object(self.adam_step, root))
