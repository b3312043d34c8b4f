"""The transducer (RNN-T) objective on the acoustic model's engine (no reference counterpart: the reference trains
with CTC).  An encoder -- engine.Engine as it is, in every arrangement it builds, its output layer projecting to the joint size J --,
a prediction network over the emitted characters -- the language model's graph: token embedding, the LSTM stack, a projection to J --
and the joint network tanh(f_t + g_u) . W_out + b_out over the T x (U+1) lattice, trained together through the lattice loss.

One flat parameter / gradient / Adam buffer holds the three parts, each starting on a 256-byte boundary under a name prefix
("encoder/", "prediction/", then joint_w and joint_b), so the global-norm clip and Adam cover every parameter in ONE
ParamStore.apply, and checkpoint.pack / unpack see one store.  Everything numeric is a libamdspeech call.
"""
import numpy as np
import torch

from . import ops
from . import stacks
from .engine import PRECISIONS, Engine, ParamLayout, ParamStore

ENCODER, PREDICTION = "encoder/", "prediction/"


class ComposedLayout(object):
    """The layouts of the parts one behind the other (every ParamLayout is a whole number of 256-byte blocks), their tensors under
    the part's prefix, then the joint's own two.  What ParamStore needs of a layout: slots, total, names(), view(), num_params()."""

    def __init__(self, parts, joint_size, num_labels):
        self.slots, self.parts, off = {}, {}, 0
        for prefix, lay in parts:
            assert lay.total % 64 == 0
            self.parts[prefix] = (off, lay)
            for name, (o, shape) in lay.slots.items():
                self.slots[prefix + name] = (off + o, shape)
            off += lay.total
        for name, shape in (("joint_w", (joint_size, num_labels)), ("joint_b", (num_labels,))):
            n = shape[0] * (shape[1] if len(shape) > 1 else 1)
            self.slots[name] = (off, shape)
            off += (n + 63) // 64 * 64
        self.total = off

    names = ParamLayout.names
    view = ParamLayout.view
    num_params = ParamLayout.num_params

    def part(self, prefix, flats):
        """The slices of the flat buffers that are the part's own store."""
        off, lay = self.parts[prefix]
        return tuple(t[off:off + lay.total] for t in flats)


class PredictionEngine(ParamStore):
    """The prediction network: language_model.LmEngine's graph up to its output layer, which projects to the joint size instead
    of the alphabet -- ParamLayout(L, H, C, J), rows tok [B, U+2] = [C-1, y_1 .. y_n, C-1, ..] of n + 1 positions, g = logits
    [U+1, B, J].  Always from the zero state."""

    def __init__(self, num_layers, hidden, num_labels, joint_size, batch_size, max_U, precision="f32", seed=1234, device="cuda",
                 storage=None):
        self.L, self.H, self.V, self.J = num_layers, hidden, num_labels, joint_size
        self.B, self.T = batch_size, max_U + 1
        ParamStore.__init__(self, ParamLayout(num_layers, hidden, num_labels, joint_size), device, storage)
        self.stack = stacks.UniStack(self, self.T, batch_size, hidden, num_layers, PRECISIONS[precision])
        self.logits = torch.empty(self.T, batch_size, joint_size, device=self.device)
        self.dlogits = torch.empty_like(self.logits)
        self._ran = False                # no launch of the stack yet: its workspace holds no status to read
        self.init_parameters(seed)

    def check(self):
        """As ParamStore.check, once the stack has run: a model that only decodes (greedy_decode steps the cells through
        ops.lm_step_state) never launches it, and the status words of a workspace no launch has armed are not a status."""
        if self._ran:
            ParamStore.check(self)

    def _describe(self):
        return "the prediction network (L=%d, H=%d, C=%d, J=%d)" % (self.L, self.H, self.V, self.J)

    def forward(self, tok, lengths, keep_in=1.0, keep_out=1.0, seed=0, training=False, per_diagonal=False):
        self.stack.lay_out(self.T, keep_in, keep_out, seed)
        ops.embed_fwd(tok, lengths, self.p("input_w"), self.p("input_b"), self.stack.z0)
        self.stack.forward(lengths, None, None, training, per_diagonal)
        self._ran = True
        self._output_fwd(self.stack.tops(lengths), self.T)
        return self.logits

    def backward(self, tok, lengths, per_diagonal=False):
        """From self.dlogits (the joint's dg): the projection, the stack and the embedding, added to the gradient buffer."""
        self._output_bwd(self.stack.tops(lengths), self.T)
        self.stack.backward(lengths, per_diagonal)
        ops.embed_bwd(tok, lengths, self.stack.dz0, self.g("input_w"), self.g("input_b"))


class TransducerEngine(ParamStore):
    """What AcousticModel uses of an engine, for the transducer objective.  `encoder` takes Engine's keyword arguments (normalization,
    precision, bidirectional, lookahead, conv, ..)."""

    def __init__(self, num_layers, hidden, input_dim, num_labels, batch_size, max_T, max_U, joint_size=512, pred_layers=1,
                 pred_hidden=None, device="cuda", seed=1234, precision="f32", **encoder):
        if not torch.cuda.is_available():
            raise RuntimeError("rnn_speech_amd needs a ROCm GPU (MI355X); there is no CPU path")
        pred_hidden = hidden if pred_hidden is None else pred_hidden
        self.C, self.J, self.B, self.U = num_labels, joint_size, batch_size, max_U
        enc_layout = self._encoder_layout(num_layers, hidden, input_dim, joint_size, max_T, encoder)
        pred_layout = ParamLayout(pred_layers, pred_hidden, num_labels, joint_size)
        ParamStore.__init__(self, ComposedLayout([(ENCODER, enc_layout), (PREDICTION, pred_layout)], joint_size, num_labels), device)
        flats = (self.params, self.grads, self.adam_m, self.adam_v)
        self.encoder = Engine(num_layers, hidden, input_dim, joint_size, batch_size, max_T, max_U, device=device, seed=seed,
                              precision=precision, storage=self.layout.part(ENCODER, flats), **encoder)
        assert self.encoder.layout.total == enc_layout.total and self.encoder.layout.slots == enc_layout.slots
        self.prediction = PredictionEngine(pred_layers, pred_hidden, num_labels, joint_size, batch_size, max_U, precision=precision,
                                           seed=seed + 1, device=device, storage=self.layout.part(PREDICTION, flats))
        self.T, self.H, self.L = self.encoder.T, hidden, num_layers
        ops.rnnt_plan(self.T, batch_size, max_U, joint_size, num_labels)      # a shape the kernels refuse raises here, with its limit
        self.lattice = torch.empty(batch_size * self.T * (max_U + 1) * num_labels, device=self.device)      # logits, then dlogits in place
        self.ws = ops.rnnt_workspace(self.T, batch_size, max_U, joint_size, num_labels, self.device)
        self.loss = torch.zeros(batch_size, device=self.device)
        self._labels = None              # (targets, n, tok, tok_len) of the mini-batch in flight
        self._init_joint(seed + 2)

    @staticmethod
    def _encoder_layout(num_layers, hidden, input_dim, joint_size, max_T, kw):
        """The encoder's ParamLayout as Engine derives it from its keyword arguments (the front convolution changes the input
        Linear's width); Engine's own layout is compared with it after construction."""
        conv = tuple(int(v) for v in kw["conv"]) if kw.get("conv") else None
        if conv:
            _, input_dim = ops.conv2d_out_shape(max_T, input_dim // conv[5], conv[0], conv[3], conv[4])
        bidir = bool(kw.get("bidirectional"))
        return ParamLayout(num_layers, hidden, input_dim, joint_size, bidirectional=bidir,
                           bidirectional_mode=kw.get("bidirectional_mode", "top") if bidir else "top",
                           lookahead=int(kw.get("lookahead", 0)), conv=conv)

    def _init_joint(self, seed):
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        lim = (6.0 / (self.J + self.C)) ** 0.5
        self.p("joint_w").copy_((torch.rand(self.J, self.C, generator=gen) * 2.0 - 1.0) * lim)
        self.p("joint_b").zero_()

    def init_parameters(self, seed=1234):
        self.encoder.init_parameters(seed)
        self.prediction.init_parameters(seed + 1)
        self._init_joint(seed + 2)

    def _describe(self):
        return "the transducer (%s; %s; J=%d)" % (self.encoder._describe(), self.prediction._describe(), self.J)

    # ---- what AcousticModel reads of an engine -------------------------------------------------------------------------------
    logits = property(lambda self: self.encoder.logits)           # the encoder projection f [T, B, J]
    stream = property(lambda self: self.encoder.stream)
    on_stream = property(lambda self: self.encoder.on_stream)
    state_h = property(lambda self: self.encoder.state_h)
    state_c = property(lambda self: self.encoder.state_c)
    layerwise = property(lambda self: self.encoder.layerwise)

    def check(self):
        self.encoder.check()
        self.prediction.check()

    def keep_state(self):
        self.encoder.keep_state()

    def zero_state(self):
        self.encoder.zero_state()

    def final_state(self):
        return self.encoder.final_state()

    def model_lengths(self, lengths):
        return self.encoder.model_lengths(lengths)

    def kernel_path(self):
        return dict(self.encoder.kernel_path(), objective="transducer", prediction=self.prediction.stack.kernel_path())

    def all_reduce_grads(self):
        from . import dataparallel
        if dataparallel.current().world > 1:
            raise ValueError("objective : transducer trains on one data-parallel rank")

    def forward(self, x, lengths, keep_in=1.0, keep_out=1.0, seed=0, use_state=False, max_len=None, training=False, per_diagonal=False,
                after_lstm=None, dense_labels=None):
        """The encoder's forward: f [T, B, J] (its logits buffer).  No labels reach it, so its fused CTC head is never taken."""
        return self.encoder.forward(x, lengths, keep_in, keep_out, seed, use_state, max_len, after_lstm=after_lstm, training=training,
                                    per_diagonal=per_diagonal)

    def _lattice(self, Tr):
        return self.lattice[:self.B * Tr * (self.U + 1) * self.C].view(self.B, Tr, self.U + 1, self.C)

    def mini_batch(self, x, lengths, dense_labels, keep_in=1.0, keep_out=1.0, seed=0, use_state=False, compute_gradients=True,
                   max_len=None, beside_ctc=None, marks=None, beside_forward=None, per_diagonal=False):
        """Encoder forward -> targets -> prediction forward -> joint -> lattice loss (dlogits in place of the logits) -> joint
        backward (df into the encoder's dlogits, dg into the prediction network's) -> prediction backward -> encoder backward.  Both
        side-work hooks of Engine.mini_batch are placed behind the two forward recurrences and joined in front of the two backward ones."""
        enc, pred = self.encoder, self.prediction
        if tuple(dense_labels.shape) != (self.B, self.U):
            raise ValueError("transducer: dense_labels %s, expected (%d, %d)" % (tuple(dense_labels.shape), self.B, self.U))

        def mark(name):
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(torch.cuda.current_stream(self.device))
                marks.append((name, ev))

        mark("begin")
        self.forward(x, lengths, keep_in, keep_out, seed, use_state, max_len, training=compute_gradients, per_diagonal=per_diagonal)
        mark("forward")
        Tr = enc._Tr
        mlen = enc.model_lengths(lengths)
        targets, n, tok, tok_len = self._labels = ops.rnnt_targets(dense_labels.contiguous(), self.C)
        g = pred.forward(tok, tok_len, keep_in, keep_out, seed + 1, training=compute_gradients, per_diagonal=per_diagonal)
        # the side work goes beside the joint and the lattice (plain launches that fill the chip or 2 B workgroups of latency), never
        # beside a recurrence: behind both forward recurrences, joined in front of both backward ones
        cur = torch.cuda.current_stream(self.device)
        after = torch.cuda.Event()
        after.record(cur)
        pending = [ev for ev in (h(after) for h in (beside_ctc, beside_forward) if h is not None) if ev is not None]
        f = enc.logits[:Tr]
        lat = self._lattice(Tr)
        ops.rnnt_joint_fwd(f, g, self.p("joint_w"), self.p("joint_b"), mlen, n, logits=lat)
        ops.rnnt_loss_fwd_bwd(lat, targets, n, mlen, loss=self.loss, dlogits=lat, ws=self.ws)
        mark("ctc")
        if not compute_gradients:
            for ev in pending:
                cur.wait_event(ev)
            return self.loss
        ops.rnnt_joint_bwd(lat, f, g, self.p("joint_w"), mlen, n, self.g("joint_w"), self.g("joint_b"), df=enc.dlogits[:Tr],
                           dg=pred.dlogits, ws=self.ws)
        if Tr < enc.T:
            enc.dlogits[Tr:].zero_()
        for ev in pending:
            cur.wait_event(ev)
        pred.backward(tok, tok_len, per_diagonal)
        enc.backward(x, lengths, per_diagonal=per_diagonal)
        mark("backward")
        return self.loss

    def greedy_decode(self, lengths):
        """Time-synchronous greedy decoding of the LAST forward's encoder output, on the device: (ids [B, U], out_len [B]) int32
        device tensors.  T_run + U iterations of ops.rnnt_greedy_step and ops.lm_step_state; nothing is read in between."""
        enc, pred = self.encoder, self.prediction
        B, U, C, Tr = self.B, self.U, self.C, enc._Tr
        dev, i32 = self.device, torch.int32
        pool_h = torch.zeros(2 * B, pred.L, pred.H, device=dev)
        pool_c = torch.zeros(2 * B, pred.L, pred.H, device=dev)
        first = torch.arange(0, 2 * B, 2, device=dev, dtype=i32)
        parent = torch.full((B,), -1, device=dev, dtype=i32)
        token = torch.full((B,), C - 1, device=dev, dtype=i32)
        dest, slot = first.clone(), first.clone()
        t_idx, m = torch.zeros(B, device=dev, dtype=i32), torch.zeros(B, device=dev, dtype=i32)
        ids = torch.zeros(B, U, device=dev, dtype=i32)
        lay = pred.layout

        def step():
            ops.lm_step_state(parent, token, dest, pool_h, pool_c, pred.p("input_w"), pred.p("input_b"), pred.p("kernel_0"),
                              lay.kernel_stride, pred.p("bias_0"), lay.bias_stride, C)

        step()                           # the start symbol (the EOS id) from the zero state
        f, mlen = enc.logits[:Tr], enc.model_lengths(lengths)
        for _ in range(Tr + U):
            ops.rnnt_greedy_step(f, mlen, U, pool_h, pred.p("output_w"), pred.p("output_b"), self.p("joint_w"), self.p("joint_b"),
                                 t_idx, m, slot, ids, parent, token, dest)
            step()
        return ids, m



# ---------------------------------------------------------------------------------------------------------------- the model
from .acoustic_model import AcousticModel  # noqa: E402  (the model class sits on the engine above)


def check_options(hyper_params, training):
    """What objective : transducer does not do, each refused by the name of its key (hyperparams.read_config_file's dict).
    train_decoder is only read by a training model."""
    get = hyper_params.get
    if training and get("train_decoder", "greedy") == "beam":
        raise ValueError("train_decoder : beam with objective : transducer -- the transducer decodes greedily on the GPU "
                         "(there is no transducer beam search); set train_decoder : greedy")
    if get("lm_weight", 0) > 0:
        raise ValueError("lm_weight : %g with objective : transducer -- language-model rescoring and fusion read CTC posteriors; "
                         "set lm_weight : 0" % get("lm_weight"))
    if get("decode_blank_skip", 0) > 0:
        raise ValueError("decode_blank_skip : %g with objective : transducer -- blank-frame skipping is a CTC beam decoder's input "
                         "stage; set decode_blank_skip : 0" % get("decode_blank_skip"))
    from . import dataparallel
    if dataparallel.current().world > 1:
        raise ValueError("objective : transducer on %d data-parallel ranks -- it trains on one" % dataparallel.current().world)


class TransducerModel(AcousticModel):
    """AcousticModel on a TransducerEngine (config key objective : transducer): the same training loop, dataset pipeline,
    checkpoints and inference surface; the greedy transducer decoder behind every prediction (merge_repeated does not apply: the
    transducer emits each character once).  The prediction network gets the acoustic keep probabilities."""
    joint_size, pred_layers, pred_hidden = 512, 1, None      # config keys transducer_joint_size / _pred_layers / _pred_hidden

    def _make_engine(self):
        if self.rnn_created:
            raise RuntimeError("Trying to create the acoustic RNN but it is already.")
        check_options({"train_decoder": self.train_decoder, "decode_blank_skip": self.decode_blank_skip,
                       "lm_weight": 1.0 if self.rescorer is not None else 0.0}, training=not self._forward)
        self.engine = TransducerEngine(self.num_layers, self.hidden_size, self.input_dim, self.num_labels, self.batch_size,
                                       self.max_input_seq_length, self.max_target_seq_length, joint_size=int(self.joint_size),
                                       pred_layers=int(self.pred_layers), pred_hidden=self.pred_hidden or None,
                                       precision=self.precision, normalization=bool(self.normalization),
                                       bidirectional=bool(self.bidirectional), sync_batch_norm=bool(self.sync_batch_norm),
                                       bidirectional_mode=self.bidirectional_mode, lookahead=int(self.lookahead_context), conv=self.conv)
        self.rnn_created = True

    _forward = False

    def create_forward_rnn(self):
        self._forward = True             # (a forward model never runs the training decoder: train_decoder is not read)
        return AcousticModel.create_forward_rnn(self)

    def align(self, session, inputs, input_seq_lengths, labels):
        raise ValueError("--align with objective : transducer -- forced alignment reads CTC posteriors")

    def _error_rate_launch(self, dlen, dense):
        """As AcousticModel's, with the greedy transducer decoder: (device distances [B], host truth lengths)."""
        from .acoustic_model import _truth_rows
        ids, out_len = self.engine.greedy_decode(dlen)
        truth = np.zeros_like(dense)
        tlen = np.zeros(self.batch_size, np.int32)
        for b, kept in enumerate(_truth_rows(dense[:self.batch_size], self.num_labels)):
            truth[b, :len(kept)] = kept
            tlen[b] = len(kept)
        dev = self.engine.device
        return ops.edit_distance(ids, out_len, torch.as_tensor(truth).to(dev), torch.as_tensor(tlen).to(dev)), tlen

    def _decode(self, dlen):
        """Dense int32 prediction matrix [B, width] padded with num_labels."""
        if self.rescorer is not None:
            raise ValueError("lm_weight > 0 with objective : transducer -- language-model rescoring and fusion read CTC posteriors")
        ids, out_len = (t.cpu().numpy() for t in self.engine.greedy_decode(dlen))
        ids = np.where(np.arange(ids.shape[1])[None, :] < out_len[:, None], ids, self.num_labels).astype(np.int32)
        return ids[:, :max(int(out_len.max()), 1)]
