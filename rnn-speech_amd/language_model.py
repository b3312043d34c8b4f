"""Character language model over the acoustic model's label alphabet: GPU training, n-best rescoring and first-pass fusion.

Stands where the reference's models/LanguageModel.py stands ("acoustic RNN -> character level RNN-LM") and keeps its class
surface where that means something here.  Next-token model, V = C = len(char_map): a sentence with tokens y_0 .. y_{n-1} is one
row tok = [C-1, y_0, .., y_{n-1}, C-1] -- the EOS / blank id C-1 doubles as the start symbol --, the input at step t is tok[t],
the target tok[t+1], lengths[b] = n + 1 predicted positions.  (A DEVIATION from the reference's stub, which trained with CTC on
shifted labels and never predicted the first token: DESIGN.md 7.)

Graph: token -> row of input_w [V,H] + input_b -> the LSTM stack of the acoustic model (ops.LstmWorkspace / lstm_fwd / lstm_bwd,
dropout as in DropoutWrapper, zero initial state for every batch: rows are independent sentences) -> output Linear [H,V] ->
log-softmax -> NLL.  Parameter names and the flat layout are engine.ParamLayout(L, H, V, V), so the numpy oracle applies unchanged
with one-hot input.  Everything numeric is a libamdspeech call; there is no torch compute and no CPU path.
"""
import logging
import os

import numpy as np
import torch

from . import checkpoint
from . import labels as _labels
from . import ops
from . import stacks
from .engine import PRECISIONS, ParamLayout, ParamStore


class LmEngine(ParamStore):
    """The op sequence of one language-model mini-batch on the parameter store of the acoustic engine (engine.ParamStore: flat
    parameter / gradient / Adam buffers, the optimiser step, healthy())."""

    def __init__(self, num_layers, hidden, num_labels, batch_size, max_len, precision="f32", seed=1234, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("rnn_speech_amd needs a ROCm GPU (MI355X); there is no CPU path")
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % ", ".join(sorted(PRECISIONS)))
        self.L, self.H, self.V = num_layers, hidden, num_labels
        self.B, self.T = batch_size, max_len
        self.precision = precision
        ParamStore.__init__(self, ParamLayout(num_layers, hidden, num_labels, num_labels), device)
        self.stack = stacks.UniStack(self, max_len, batch_size, hidden, num_layers, PRECISIONS[precision])
        self.logits = torch.empty(max_len, batch_size, num_labels, device=self.device)
        self.dlogits = torch.empty_like(self.logits)
        self.nll = torch.zeros(max_len, batch_size, device=self.device)
        self.loss = torch.zeros(batch_size, device=self.device)
        self._Tr = max_len               # steps the last forward visited
        self.init_parameters(seed)

    def _describe(self):
        return "the language model (L=%d, H=%d, V=%d)" % (self.L, self.H, self.V)

    # ---- one mini-batch ----------------------------------------------------------------
    def _check_batch(self, tok, lengths):
        if tuple(tok.shape[:1]) != (self.B,) or tok.shape[1] < self.T + 1 or lengths.numel() != self.B:
            raise ValueError("language model batch: tok %s / lengths %s do not fit B = %d rows of %d + 1 tokens"
                             % (tuple(tok.shape), tuple(lengths.shape), self.B, self.T))

    def forward(self, tok, lengths, keep_in=1.0, keep_out=1.0, seed=0, max_len=None, training=False, per_diagonal=False):
        """tok int32 [B, >= T+1] device, lengths int32 [B] device -> logits [T,B,V] (the engine's buffer; rows past the run length
        are the output bias)."""
        self._check_batch(tok, lengths)
        Tr = self._Tr = self._run_length(max_len)
        self.stack.lay_out(Tr, keep_in, keep_out, seed)
        ops.embed_fwd(tok, lengths, self.p("input_w"), self.p("input_b"), self.stack.z0)
        self.stack.forward(lengths, None, None, training, per_diagonal)      # (zero initial state: rows are independent sentences)
        self._output_fwd(self.stack.tops(lengths), Tr)
        self._fill_tail(Tr)
        return self.logits

    def mini_batch(self, tok, lengths, keep_in=1.0, keep_out=1.0, seed=0, max_len=None, scale=1.0, compute_gradients=True,
                   per_diagonal=False):
        """embed_fwd -> lstm_fwd -> output Linear -> xent_fwd_bwd -> output Linear backward (dZ_top in the workspace) -> lstm_bwd ->
        embed_bwd.  The gradient ADDED to self.grads is `scale` times that of the SUM of the NLL over tokens and rows; self.loss [B]
        and self.nll [T,B] are unscaled.  per_diagonal: the repeat of a mini-batch whose whole-sequence launch timed out."""
        self.forward(tok, lengths, keep_in, keep_out, seed, max_len, training=compute_gradients, per_diagonal=per_diagonal)
        stack, Tr = self.stack, self._Tr
        targets = tok[:, 1:]
        if Tr < self.T:
            self.nll[Tr:].zero_()
        ops.xent_fwd_bwd(self.logits[:Tr], targets, lengths, scale=scale, nll=self.nll[:Tr], loss=self.loss,
                         dlogits=self.dlogits[:Tr] if compute_gradients else None, want_grad=compute_gradients)
        if not compute_gradients:
            return self.loss
        self._output_bwd(stack.tops(lengths), Tr)
        stack.backward(lengths, per_diagonal)
        ops.embed_bwd(tok, lengths, stack.dz0, self.g("input_w"), self.g("input_b"))
        return self.loss

    def mini_batch_recovering(self, tok, lengths, kept_grads=None, compute_gradients=True, **kw):
        """mini_batch() that survives a dataflow time-out: when a whole-sequence launch gave up waiting, the gradient buffer goes
        back to `kept_grads` (None: to zero -- the first mini-batch of an optimiser step), the mini-batch runs again on the
        launch-per-diagonal kernels and check() has to pass.  Returns True when it had to do that."""
        self.mini_batch(tok, lengths, compute_gradients=compute_gradients, **kw)
        if self.healthy():
            return False
        if compute_gradients:
            self.grads.copy_(kept_grads) if kept_grads is not None else self.zero_grads()
        self.mini_batch(tok, lengths, compute_gradients=compute_gradients, per_diagonal=True, **kw)
        self.check()
        return True

    def score(self, tok, lengths, max_len=None, per_token=False):
        """Forward only, at keep 1.0: -loss[b], the natural-log probability of each row including its closing EOS, as a host
        array [B]; with per_token the -nll [T,B] too."""
        self.mini_batch_recovering(tok, lengths, max_len=max_len, compute_gradients=False)
        logp = -self.loss.cpu().numpy()
        return (logp, -self.nll.cpu().numpy()) if per_token else logp

    def kernel_path(self):
        """The LSTM path of the LAST forward and of the backward that belongs to it, named as Engine.kernel_path names them."""
        return dict(self.stack.kernel_path(), run_length=self._Tr)


def sentence_rows(id_lists, num_labels, width=None):
    """Token-id lists (without start / end symbols) -> (tok int32 [n, width + 1], lengths int32 [n]) with tok[b] = [C-1, ids.., C-1]
    padded with C-1 and lengths[b] = len(ids) + 1; width defaults to the longest row's length."""
    eos = num_labels - 1
    lens = np.array([len(ids) + 1 for ids in id_lists], np.int32)
    width = int(lens.max()) if width is None and len(lens) else int(width or 1)
    tok = np.full((len(id_lists), width + 1), eos, np.int32)
    for b, ids in enumerate(id_lists):
        if len(ids) + 1 > width:
            raise ValueError("sentence of %d tokens does not fit rows of %d" % (len(ids), width))
        tok[b, 1:1 + len(ids)] = ids
    return tok, lens


class LanguageModel(checkpoint.TrainedModel):
    """The reference class's surface on the GPU engine.  `session` arguments are accepted and ignored, as in AcousticModel."""

    def __init__(self, num_layers, hidden_size, batch_size, max_input_seq_length, max_target_seq_length, input_dim,
                 precision="f32", seed=1234):
        self.num_layers, self.hidden_size, self.batch_size = num_layers, hidden_size, batch_size
        self.max_input_seq_length, self.max_target_seq_length = max_input_seq_length, max_target_seq_length
        self.input_dim = self.num_labels = input_dim          # the output has the input's dimension
        self.precision, self.seed = precision, seed
        checkpoint.TrainedModel.__init__(self)
        self.recovered_steps = 0
        self._dataset = self._iter = None
        self._dropout_seed = 0
        self._mini_batch_size = 1      # mini-batches per optimiser step (run_train_step sets it): the gradient is their mean
        self._reset_accumulators()

    # rows hold max_target_seq_length tokens plus the closing EOS
    @property
    def _row_len(self):
        return self.max_target_seq_length + 1

    def _create(self):
        if self.rnn_created:
            logging.fatal("Trying to create the language RNN but it is already.")
        self.engine = LmEngine(self.num_layers, self.hidden_size, self.num_labels, self.batch_size, self._row_len,
                               precision=self.precision, seed=self.seed)
        self.rnn_created = True

    def create_forward_rnn(self):
        self._create()

    def create_training_rnn(self, input_keep_prob, output_keep_prob, grad_clip, learning_rate, lr_decay_factor, use_iterator=False):
        self._create()
        self._set_training(input_keep_prob, output_keep_prob, grad_clip, learning_rate, lr_decay_factor)

    # ---- data ------------------------------------------------------------------------------
    @staticmethod
    def build_dataset(input_set, batch_size, max_input_seq_length, char_map):
        """Sentences -> a list of (tok int32 [batch_size, max_input_seq_length + 2], lengths int32 [batch_size], n_rows) batches:
        rows [C-1, ids.., C-1] of labels.get_str_labels, padded with C-1; the last batch is padded with empty rows (length 0).
        Sentences of more than max_input_seq_length tokens are skipped, with a logged count."""
        C_ = len(char_map)
        rows, skipped = [], 0
        for text in input_set:
            ids = _labels.get_str_labels(char_map, text, add_eos=False)
            if len(ids) > max_input_seq_length:
                skipped += 1
                continue
            rows.append(ids)
        if skipped:
            logging.warning("language model dataset: %d of %d sentences are longer than %d tokens and were skipped",
                            skipped, len(input_set), max_input_seq_length)
        batches = []
        for i in range(0, len(rows), batch_size):
            chunk = rows[i:i + batch_size]
            tok, lens = sentence_rows(chunk, C_, width=max_input_seq_length + 1)
            pad = batch_size - len(chunk)
            if pad:
                tok = np.concatenate([tok, np.full((pad, tok.shape[1]), C_ - 1, np.int32)])
                lens = np.concatenate([lens, np.zeros(pad, np.int32)])
            batches.append((tok, lens, len(chunk)))
        return batches

    def add_dataset_input(self, dataset):
        self._dataset = list(dataset)
        self._iter = iter(self._dataset)
        return self

    def rewind(self):
        self._iter = iter(self._dataset)

    # ---- steps -------------------------------------------------------------------------------
    def _reset_accumulators(self):
        self._nll_sum, self._tokens, self._errors, self._mini_batches = 0.0, 0, 0, 0

    def start_batch(self, session, is_training, run_options=None, run_metadata=None):
        self._reset_accumulators()
        if is_training:
            self.engine.zero_grads()

    def _device_batch(self, tok, lens):
        dev = self.engine.device
        return torch.as_tensor(tok).to(dev), torch.as_tensor(lens).to(dev)

    def run_step(self, session, compute_gradients=True, run_options=None, run_metadata=None):
        """One mini-batch from the dataset; StopIteration when it is empty (the reference's OutOfRangeError)."""
        tok, lens, _ = next(self._iter)
        eng = self.engine
        n_tok = int(lens.sum())
        d_tok, d_len = self._device_batch(tok, lens)
        keep = (self.input_keep_prob, self.output_keep_prob) if compute_gradients else (1.0, 1.0)
        self._dropout_seed += 1
        kept = eng.grads.clone() if compute_gradients and self._mini_batches > 0 else None
        if eng.mini_batch_recovering(d_tok, d_len, kept, compute_gradients, keep_in=keep[0], keep_out=keep[1], seed=self._dropout_seed,
                                     max_len=int(lens.max()), scale=1.0 / (max(n_tok, 1) * self._mini_batch_size)):
            self.recovered_steps += 1
            if self.recovered_steps == 1:
                logging.warning("a whole-sequence LSTM launch timed out: repeating the mini-batch on the launch-per-diagonal kernels")
        loss = eng.loss.cpu().numpy().astype(np.float64)
        # token error of the arg-max prediction: the "error rate" slot the plateau rule watches
        Tr = eng._Tr
        pred = eng.logits[:Tr].cpu().numpy().argmax(axis=2)                    # [Tr, B], on the host
        live = np.arange(Tr)[:, None] < lens[None, :]
        self._errors += int(((pred != tok[:, 1:Tr + 1].T) & live).sum())
        self._nll_sum += float(loss.sum())
        self._tokens += n_tok
        self._mini_batches += 1
        return self._mini_batches

    def end_batch(self, session, is_training, run_options=None, run_metadata=None, rnn_state_reset_ratio=1.0):
        """-> (mean NLL per token, token error rate, global step).  Training: gradients are the mean over the step's mini_batch_size mini-batches of
        the per-token mean (the scale of each xent call), clipped and applied by ops.clip_adam.  rnn_state_reset_ratio is not read: no state is carried."""
        if is_training:
            self.engine.apply(self.learning_rate_var.value, self.grad_clip)
            self.global_step.value += 1
        n = max(self._tokens, 1)
        return self._nll_sum / n, self._errors / n, self.global_step.value

    def run_train_step(self, sess, mini_batch_size, rnn_state_reset_ratio=1.0, run_options=None, run_metadata=None):
        """-> (mean_loss, mean_error_rate, current_step, dataset_empty)."""
        self._mini_batch_size = max(int(mini_batch_size), 1)
        self.start_batch(sess, True)
        dataset_empty = False
        try:
            for _ in range(mini_batch_size):
                self.run_step(sess, True)
        except StopIteration:
            dataset_empty = True
        if self._mini_batches == 0:
            return 0.0, 0.0, self.global_step.value, dataset_empty
        mean_loss, err, step = self.end_batch(sess, True)
        logging.info("Batch %d : loss %.5f - error_rate %.5f", step, mean_loss, err)
        return mean_loss, err, step, dataset_empty

    def evaluate_dataset(self, dataset):
        """(mean NLL per token, token error rate) of a build_dataset() list, forward only."""
        keep_ds, keep_it = self._dataset, self._iter
        self.add_dataset_input(dataset)
        self.start_batch(None, False)
        try:
            while True:
                self.run_step(None, False)
        except StopIteration:
            pass
        self._dataset, self._iter = keep_ds, keep_it
        loss, err, _ = self.end_batch(None, False)
        return loss, err

    # ---- scoring -------------------------------------------------------------------------------
    def score(self, id_lists):
        """Natural-log probability, closing EOS included, of each token-id list (any number of them: batched and padded here).
        A list longer than max_target_seq_length scores -inf."""
        eng = self.engine
        out = np.full(len(id_lists), -np.inf, np.float64)
        fit = [i for i, ids in enumerate(id_lists) if len(ids) <= self.max_target_seq_length]
        for s in range(0, len(fit), eng.B):
            idx = fit[s:s + eng.B]
            tok, lens = sentence_rows([id_lists[i] for i in idx], self.num_labels, width=self._row_len)
            pad = eng.B - len(idx)
            if pad:
                tok = np.concatenate([tok, np.full((pad, tok.shape[1]), self.num_labels - 1, np.int32)])
                lens = np.concatenate([lens, np.zeros(pad, np.int32)])
            d_tok, d_len = self._device_batch(tok, lens)
            logp = eng.score(d_tok, d_len, max_len=int(lens.max()))
            out[idx] = logp[:len(idx)]
        return out

    # ---- checkpoints: checkpoint_dir/language/languagemodel.npz, the reference graph's variable names + Adam state -----------
    @staticmethod
    def checkpoint_path(checkpoint_dir):
        return os.path.join(checkpoint_dir, "language", "languagemodel.npz")

    def save(self, session, checkpoint_dir):
        path = self.checkpoint_path(checkpoint_dir)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        checkpoint.write(path, checkpoint.pack(self.engine, self.global_step.value, self.learning_rate_var.value))
        logging.info("Language model checkpoint saved")

    def restore(self, session, checkpoint_dir, must_exist=False):
        path = self.checkpoint_path(checkpoint_dir)
        if not os.path.exists(path):
            if must_exist:
                raise RuntimeError("no language model checkpoint in %s (expected %s): train one with --train_language or set "
                                   "lm_weight to 0" % (os.path.dirname(path), os.path.basename(path)))
            logging.info("Created language model with fresh parameters.")
            return False
        self.global_step.value, self.learning_rate_var.value, _ = checkpoint.unpack(np.load(path), self.engine)
        return True


# ---- n-best rescoring -----------------------------------------------------------------------------
def rescore_nbest(ids, out_len, log_prob, n_found, scorer, lm_weight, lm_length_bonus=0.0):
    """Pick one hypothesis per utterance from the n-best lists of ops.ctc_beam_search_nbest (ids [B,N,T], out_len [B,N], log_prob
    [B,N], n_found [B]): drop duplicate id sequences keeping the best CTC score, score the survivors of ALL utterances in one
    scorer(list_of_id_lists) -> natural-log probabilities call, return argmax(log p_ctc + lm_weight * log p_lm + lm_length_bonus *
    n_tokens) as (ids [B,T] padded as the input pads, out_len [B], log_prob [B] -- the winner's CTC score).  With lm_weight == 0
    entry 0 comes back untouched and the scorer is not called."""
    B = ids.shape[0]
    if not lm_weight:
        return ids[:, 0].copy(), out_len[:, 0].copy(), log_prob[:, 0].copy()
    cands, owner = [], []
    for b in range(B):
        seen = set()
        for k in range(int(n_found[b])):                    # best CTC score first: the first of equal sequences is kept
            key = tuple(int(v) for v in ids[b, k, :out_len[b, k]])
            if key in seen:
                continue
            seen.add(key)
            cands.append(list(key))
            owner.append((b, k))
    lm = np.asarray(scorer(cands), np.float64) if cands else np.zeros(0)
    best = [(-np.inf, 0)] * B
    for (b, k), ids_k, lp in zip(owner, cands, lm):
        total = float(log_prob[b, k]) + lm_weight * float(lp) + lm_length_bonus * len(ids_k)
        if total > best[b][0]:
            best[b] = (total, k)
    pick = np.array([k for _, k in best])
    rows = np.arange(B)
    return ids[rows, pick].copy(), out_len[rows, pick].copy(), log_prob[rows, pick].copy()


class NbestRescorer(object):
    """What AcousticModel.rescorer holds when lm_weight > 0: decode lm_nbest paths per utterance on the host, score the distinct
    ones of the whole mini-batch with the language model on the GPU, return the winners as ops.ctc_beam_search returns its path."""

    def __init__(self, scorer, lm_weight, lm_nbest=16, lm_length_bonus=0.0):
        self.scorer, self.lm_weight, self.lm_nbest, self.lm_length_bonus = scorer, float(lm_weight), int(lm_nbest), float(lm_length_bonus)

    def __call__(self, logits, lengths, beam_width=100, merge_repeated=True):
        nbest = ops.ctc_beam_search_nbest(logits, lengths, self.lm_nbest, beam_width, merge_repeated)
        ids, out_len, _ = rescore_nbest(*nbest, scorer=self.scorer, lm_weight=self.lm_weight, lm_length_bonus=self.lm_length_bonus)
        return ids, out_len


# ---- the language model inside the beam (first-pass fusion) -----------------------------------------
class LmStepper(object):
    """The `step` of ops.ctc_beam_search_fused on the GPU: a pool of n_slots model states (two float32 device arrays [n_slots, L,
    H]) and one ops.lm_step per call.  engine_or_params: an LmEngine (its float32 master parameters are used in place, whatever
    precision it trains in) or a dict of numpy arrays under the ParamLayout(L, H, V, V) names.
    __call__(parent, token, dest) -> logq float32 [n, V] on the host: the indices go up through one pinned buffer, then one
    amdspeech_lm_step, one device-to-host copy and one stream synchronisation.  The slot contract of amdspeech_lm_step is checked
    here, on the host copies: dest distinct and inside the pool, no dest among the parents, parents -1 or inside the pool."""

    def __init__(self, engine_or_params, n_slots, max_rows=None, device="cuda"):
        if isinstance(engine_or_params, dict):
            arrays = engine_or_params
            V, H = np.shape(arrays["input_w"])
            L = sum(1 for k in arrays if k.startswith("kernel_"))
            self.layout = ParamLayout(L, H, V, V)
            self.device = torch.device(device)
            self.params = torch.zeros(self.layout.total, device=self.device)
            for name, a in arrays.items():
                self.layout.view(self.params, name).copy_(torch.as_tensor(np.asarray(a), dtype=torch.float32))
        else:
            eng = engine_or_params
            self.layout, self.params, self.device = eng.layout, eng.params, eng.device
            L, H, V = eng.L, eng.H, eng.V
        self.L, self.H, self.V, self.n_slots = int(L), int(H), int(V), int(n_slots)
        ops.lm_step_plan(1, self.L, self.H, self.V)                      # a shape the kernels refuse raises here, not in the beam
        self.pool_h = torch.zeros(self.n_slots, self.L, self.H, device=self.device)
        self.pool_c = torch.zeros_like(self.pool_h)
        self._cap = 0
        self._reserve(int(max_rows or min(self.n_slots, 4096)))
        self.calls, self.rows, self.seconds = 0, 0, 0.0                  # what tools/lm_fusion_bench.py reports

    def _reserve(self, rows):
        if rows <= self._cap:
            return
        self._cap = rows
        self._idx_host = torch.empty(3 * rows, dtype=torch.int32).pin_memory()
        self._idx_dev = torch.empty(3 * rows, dtype=torch.int32, device=self.device)
        self._logq_dev = torch.empty(rows, self.V, device=self.device)
        self._logq_host = torch.empty(rows, self.V).pin_memory()

    def _p(self, name):
        return self.layout.view(self.params, name)

    def check_slots(self, parent, dest):
        n_slots = self.n_slots
        if dest.size and (dest.min() < 0 or dest.max() >= n_slots):
            raise ValueError("lm step: a dest slot is outside 0 .. %d" % (n_slots - 1))
        if parent.size and (parent.min() < -1 or parent.max() >= n_slots):
            raise ValueError("lm step: a parent slot is outside -1 .. %d" % (n_slots - 1))
        if np.unique(dest).size != dest.size:
            raise ValueError("lm step: two rows write the same dest slot")
        if np.intersect1d(dest, parent).size:
            raise ValueError("lm step: a dest slot is also a parent slot of the same call")

    def __call__(self, parent, token, dest):
        import time
        t0 = time.perf_counter()
        parent, token, dest = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (parent, token, dest))
        n = parent.size
        if n == 0 or token.size != n or dest.size != n:
            raise ValueError("lm step: parent, token and dest must hold the same positive number of rows")
        self.check_slots(parent, dest)
        self._reserve(n)
        host = self._idx_host.numpy()
        host[:n], host[n:2 * n], host[2 * n:3 * n] = parent, token, dest
        idx = self._idx_dev[:3 * n]
        idx.copy_(self._idx_host[:3 * n], non_blocking=True)
        lay = self.layout
        ops.lm_step(idx[:n], idx[n:2 * n], idx[2 * n:], self.pool_h, self.pool_c, self._p("input_w"), self._p("input_b"),
                    self._p("kernel_0"), lay.kernel_stride, self._p("bias_0"), lay.bias_stride, self._p("output_w"), self._p("output_b"),
                    logq=self._logq_dev)
        self._logq_host[:n].copy_(self._logq_dev[:n], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = self._logq_host[:n].numpy().copy()
        self.calls += 1
        self.rows += n
        self.seconds += time.perf_counter() - t0
        return out


class FusedDecoder(object):
    """What AcousticModel.rescorer holds at lm_fusion : beam: NbestRescorer's call signature, the language model INSIDE the beam
    (ops.ctc_beam_search_fused over an LmStepper).  The model scores the prefix as decoded, before merge_repeated.  model: a
    LanguageModel, an LmEngine or a parameter dict.  The stepper (state pool and staging) is made at the first call and kept while
    the mini-batch size and the beam width stay the same."""

    def __init__(self, model, lm_weight, beam_width=100, lm_length_bonus=0.0, max_threads=0):
        self.source = getattr(model, "engine", model)
        self.lm_weight, self.beam_width, self.lm_length_bonus = float(lm_weight), int(beam_width), float(lm_length_bonus)
        self.max_threads = int(max_threads)
        self.stepper = None

    def _stepper(self, B, beam_width):
        n_slots = ops.ctc_beam_search_fused_slots(B, beam_width)
        if self.stepper is None or self.stepper.n_slots != n_slots:
            self.stepper = LmStepper(self.source, n_slots, max_rows=B * beam_width + 1)
        return self.stepper

    def __call__(self, logits, lengths, beam_width=None, merge_repeated=True):
        width = self.beam_width if beam_width is None else int(beam_width)
        B = logits.shape[1]
        ids, out_len, _ = ops.ctc_beam_search_fused(logits, lengths, self._stepper(B, width), 0, width, merge_repeated, self.lm_weight,
                                                    self.lm_length_bonus, max_threads=self.max_threads)
        return ids, out_len
