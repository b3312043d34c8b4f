"""Torch-tensor front of the C ABI: every function takes CUDA (ROCm) float32/int32
tensors, hands their device pointers and the current HIP stream to
libamdspeech.so, and returns tensors.  Torch is only the allocator / stream
provider here; there is no torch compute and no CPU fallback.
"""
import ctypes as C
import os

import torch

from . import lib as _l

MODE_MFCC, MODE_FBANK = 0, 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("expected a contiguous float32 device tensor, got %s %s" % (t.dtype, t.device))


def _chk_f32_rows(*ts):
    """2-D float32 device matrices whose ROWS are contiguous (a column slice of a wider buffer is fine: ld = stride(0))."""
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
            raise ValueError("expected a float32 device matrix with contiguous rows, got %s %s %s" % (t.dtype, t.device, t.stride()))


def _chk_i32(*ts):
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError("expected a contiguous int32 device tensor")


def _chk_f32_3d(what, x, dims):
    """x is a contiguous float32 device tensor of three dimensions (`dims` names them in the message); returns its shape."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError("%s: expected a contiguous float32 device tensor %s, got %s"
                         % (what, dims, (x.dtype, x.device, tuple(x.shape), x.stride()) if torch.is_tensor(x) else type(x)))
    return x.shape


def _c_ints(values, B, what):
    """One C int per row from python ints."""
    if len(values) != B:
        raise ValueError("%s: %d values for %d rows" % (what, len(values), B))
    return (C.c_int * max(B, 1))(*[int(v) for v in values])


def _plan_dict(info):
    """A plan struct of lib.py as a dict of ints."""
    return {name: int(getattr(info, name)) for name, _ in info._fields_}


def _gemm_dims(a_shape, b_shape, trans_a, trans_b):
    """(M, N, K) of op(A) @ op(B) from the (rows, cols) of the two operands as stored."""
    M, K = (a_shape[1], a_shape[0]) if trans_a else a_shape
    K2, N = (b_shape[1], b_shape[0]) if trans_b else b_shape
    assert K == K2, (tuple(a_shape), tuple(b_shape))
    return M, N, K


def _cached_ws(cache, key, nbytes):
    """The uint8 device workspace cached under key (its last element is the device); nbytes() sizes a new one.  A cache holds the
    few shapes a job alternates between: past 8 entries it starts again."""
    ws = cache.get(key)
    if ws is None:
        if len(cache) > 8:
            cache.clear()
        ws = cache[key] = torch.empty(nbytes(), device=key[-1], dtype=torch.uint8)
    return ws


# ------------------------------------------------------------------ GEMM / Linear
def gemm(a, b, trans_a=False, trans_b=False, bias=None, out=None, accumulate=False):
    """C = op(A) @ op(B) (+ bias).  a is [M,K] (or [K,M] if trans_a), b [K,N] (or [N,K])."""
    _chk_f32(bias)
    _chk_f32_rows(a, b, out)
    M, N, K = _gemm_dims(a.shape, b.shape, trans_a, trans_b)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _l.check(_l.load().amdspeech_gemm_f32(_stream(), int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0),
                                          _p(b), b.stride(0), _p(out), out.stride(0), _p(bias), int(accumulate)),
             "gemm_f32")
    return out


def gemm_bf16x3(a, b, trans_a=False, trans_b=False, bias=None, out=None, accumulate=False, single=False):
    """The same product as gemm() in split precision (bf16 hi/lo pairs, three bf16 MFMAs per product term, f32 accumulate);
    single=True: plain bf16 operands (one bf16 per value, one MFMA per term: precision = "bf16")."""
    _chk_f32(bias)
    _chk_f32_rows(a, b, out)
    M, N, K = _gemm_dims(a.shape, b.shape, trans_a, trans_b)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    fn = _l.load().amdspeech_gemm_bf16 if single else _l.load().amdspeech_gemm_bf16x3
    _l.check(fn(_stream(), int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), _p(bias),
                int(accumulate)), "gemm_bf16" if single else "gemm_bf16x3")
    return out


def gemm_bf16(a, b, **kw):
    return gemm_bf16x3(a, b, single=True, **kw)


def _plan_operand(x):
    """(address, rows, cols, ld) of an operand of gemm_plan: a tensor, or (rows, cols), (rows, cols, ld), (rows, cols, ld, address) --
    the address is only looked at for null and alignment (default: a nominal 16-byte aligned one)."""
    if torch.is_tensor(x):
        return x.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
    x = tuple(int(v) for v in x)
    rows, cols = x[:2]
    return (x[3] if len(x) > 3 else 4096), rows, cols, (x[2] if len(x) > 2 else cols)


def gemm_plan(a, b, trans_a=False, trans_b=False, bias=None, out=None, accumulate=False, colsum=False, count=1, precision=0):
    """The kernel gemm() (precision 0), gemm_bf16x3() (1) or gemm_bf16() (2) takes for a product and its launch geometry
    (amdspeech.h: amdspeech_gemm_plan), as a dict of ints with "family" as a name (lib.GEMM_FAMILIES).  Nothing is launched.
    a, b, out: tensors, or shapes as _plan_operand takes them (out=None: a contiguous, aligned result); bias: a tensor, an
    address, True (an aligned one) or None; colsum: with linear_bwd's fused column sums; count >= 2: gemm_tn_group()."""
    pa, ar, ac, lda = _plan_operand(a)
    pb, br, bc, ldb = _plan_operand(b)
    M, N, K = _gemm_dims((ar, ac), (br, bc), trans_a, trans_b)
    pc, _, _, ldc = _plan_operand(out if out is not None else (M, N))
    pbias = 0 if bias is None or bias is False else (4096 if bias is True else (bias.data_ptr() if torch.is_tensor(bias) else int(bias)))
    info = _l.GemmPlanInfo()
    _l.check(_l.load().amdspeech_gemm_plan(int(precision), int(trans_a), int(trans_b), M, N, K, C.c_void_p(pa), lda, C.c_void_p(pb), ldb,
                                           C.c_void_p(pc), ldc, C.c_void_p(pbias), int(accumulate), int(colsum), int(count), C.byref(info)),
             "gemm_plan")
    plan = _plan_dict(info)
    plan["family"] = _l.GEMM_FAMILIES[plan["family"]]
    return plan


def gemm_tn_group(a, b, out, colsum=None, accumulate=False):
    """out[i] (+)= a[i]^T @ b[i] for up to lib.GEMM_GROUP_MAX problems of one shape in ONE launch (amdspeech_gemm_f32_tn_group: the
    weight gradients of an LSTM backward pass); a[i] [K,M], b[i] [K,N], out[i] [M,N] with contiguous rows.  colsum: None, or a list with
    a [N] tensor (+= column sums of b[i]) or None per problem.  A shape the kernel does not take raises."""
    count = len(a)
    assert count == len(b) == len(out) and (colsum is None or len(colsum) == count)
    _chk_f32_rows(*a, *b, *out)
    K, M = a[0].shape
    N = b[0].shape[1]
    for x, y, z in zip(a, b, out):
        assert tuple(x.shape) == (K, M) and tuple(y.shape) == (K, N) and tuple(z.shape) == (M, N)
        assert x.stride(0) == a[0].stride(0) and y.stride(0) == b[0].stride(0) and z.stride(0) == out[0].stride(0)
    if colsum is not None:
        _chk_f32(*colsum)
    arr = lambda ts: (C.c_void_p * count)(*[t.data_ptr() if t is not None else None for t in ts])
    _l.check(_l.load().amdspeech_gemm_f32_tn_group(_stream(), count, M, N, K, arr(a), a[0].stride(0), arr(b), b[0].stride(0), arr(out),
                                                   out[0].stride(0), arr(colsum) if colsum is not None else None, int(accumulate)),
             "gemm_f32_tn_group")
    return out


def colsum_accumulate(x, out):
    """out[c] += sum_r x[r, c] (amdspeech_colsum_accumulate); x [rows, cols] with contiguous rows."""
    _chk_f32_rows(x)
    _chk_f32(out)
    assert out.numel() == x.shape[1]
    _l.check(_l.load().amdspeech_colsum_accumulate(_stream(), _p(x), x.shape[0], x.shape[1], x.stride(0), _p(out)), "colsum_accumulate")
    return out


def gemm_bf16_packed(a, b, trans_a=False, trans_b=False, bias=None, out=None, accumulate=False, scratch=None):
    """The plain-bf16 product through bf16 COPIES of the operands (amdspeech_gemm_bf16_packed: what the H = 1024 LSTM path runs at
    precision = "bf16").  Returns None when the shape is not taken (the caller then uses gemm_bf16).  scratch: a uint8 device tensor
    used as given (256-byte aligned, at least the bytes amdspeech_gemm_bf16_packed_scratch_bytes names); None allocates one."""
    _chk_f32(bias)
    _chk_f32_rows(a, b, out)
    M, N, K = _gemm_dims(a.shape, b.shape, trans_a, trans_b)
    lib = _l.load()
    n = lib.amdspeech_gemm_bf16_packed_scratch_bytes(int(trans_a), int(trans_b), M, N, K, a.stride(0), b.stride(0))
    if n == 0:
        return None
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty(n, device=a.device, dtype=torch.uint8)
    if not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= n and scratch.data_ptr() % 256 == 0):
        raise ValueError("scratch: expected a contiguous uint8 device tensor of >= %d bytes, 256-byte aligned" % n)
    _l.check(lib.amdspeech_gemm_bf16_packed(_stream(), int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out),
                                            out.stride(0), _p(bias), int(accumulate), _p(scratch), scratch.numel()), "gemm_bf16_packed")
    return out


def gemm_bf16_packed_plan(a, b, trans_a=False, trans_b=False):
    """The plan of gemm_bf16_packed()'s product kernel (amdspeech.h: amdspeech_gemm_bf16_packed_plan), as gemm_plan() returns one:
    family "bf16p".  a, b: tensors or shapes as _plan_operand takes them.  A shape that is not taken raises."""
    _, ar, ac, lda = _plan_operand(a)
    _, br, bc, ldb = _plan_operand(b)
    M, N, K = _gemm_dims((ar, ac), (br, bc), trans_a, trans_b)
    info = _l.GemmPlanInfo()
    _l.check(_l.load().amdspeech_gemm_bf16_packed_plan(int(trans_a), int(trans_b), M, N, K, lda, ldb, C.byref(info)), "gemm_bf16_packed_plan")
    plan = _plan_dict(info)
    plan["family"] = _l.GEMM_FAMILIES[plan["family"]]
    return plan


def _chk_bf16_rows(*ts):
    """2-D device matrices of bf16 values (torch.bfloat16, or their bits as int16) with contiguous rows."""
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype in (torch.bfloat16, torch.int16) and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
            raise ValueError("expected a bfloat16 / int16 device matrix with contiguous rows, got %s %s %s" % (t.dtype, t.device, t.stride()))


def bf16_copy(src, dst, transpose=False, colsum=None, plain=None):
    """dst = bf16(src) (amdspeech_bf16_copy: the operand copies of the packed bf16 path).  src [rows, cols] f32 with contiguous rows;
    dst [rows, cols] dense, or -- transpose -- [cols, rows] with contiguous rows; then also colsum [cols] f32 (+= column sums of src)
    and plain [rows, cols] dense (the row-major copy from the same read)."""
    _chk_f32_rows(src)
    _chk_f32(colsum)
    _chk_bf16_rows(dst, plain)
    rows, cols = src.shape
    assert tuple(dst.shape) == ((cols, rows) if transpose else (rows, cols)), (src.shape, dst.shape)
    assert colsum is None or colsum.numel() == cols
    assert plain is None or (tuple(plain.shape) == (rows, cols) and plain.is_contiguous())
    _l.check(_l.load().amdspeech_bf16_copy(_stream(), _p(src), src.stride(0), rows, cols, int(transpose), _p(dst), dst.stride(0), _p(colsum),
                                           _p(plain)), "bf16_copy")
    return dst


def bf16_transpose(src, dst):
    """dst [cols, rows] = src [rows, cols]^T in bf16 (amdspeech_bf16_transpose); src dense, dst with contiguous rows."""
    _chk_bf16_rows(src, dst)
    rows, cols = src.shape
    assert src.is_contiguous() and tuple(dst.shape) == (cols, rows), (src.shape, dst.shape)
    _l.check(_l.load().amdspeech_bf16_transpose(_stream(), _p(src), rows, cols, _p(dst), dst.stride(0)), "bf16_transpose")
    return dst


def linear_fwd(x, w, b, out=None):
    """x [M,K] @ w [K,N] + b [N]."""
    _chk_f32(x, w, b, out)
    M, K = x.shape
    N = w.shape[1]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _l.check(_l.load().amdspeech_linear_fwd(_stream(), _p(x), _p(w), _p(b), _p(out), M, K, N), "linear_fwd")
    return out


def linear_bwd(x, w, dy, dw, db, need_dx=True, dx=None):
    """dw += x^T dy, db += colsum(dy); returns dx = dy w^T (or None)."""
    _chk_f32(x, w, dy, dw, db, dx)
    M, K = x.shape
    N = w.shape[1]
    if need_dx and dx is None:
        dx = torch.empty(M, K, device=x.device, dtype=torch.float32)
    _l.check(_l.load().amdspeech_linear_bwd(_stream(), _p(x), _p(w), _p(dy), _p(dx if need_dx else None),
                                            _p(dw), _p(db), M, K, N), "linear_bwd")
    return dx if need_dx else None


# -------------------------------------------------------------------- batch norm
def batchnorm_fwd(x, y, xhat, inv_std, eps=1e-3):
    """x, y [T,B,H] (may alias); xhat [T,B,H] or None; inv_std [T,H]."""
    _chk_f32(x, y, xhat, inv_std)
    T, B, H = x.shape
    _l.check(_l.load().amdspeech_batchnorm_fwd(_stream(), _p(x), _p(y), _p(xhat), _p(inv_std), T, B, H, eps),
             "batchnorm_fwd")


def batchnorm_bwd(dy, xhat, inv_std, dx):
    _chk_f32(dy, xhat, inv_std, dx)
    T, B, H = dy.shape
    _l.check(_l.load().amdspeech_batchnorm_bwd(_stream(), _p(dy), _p(xhat), _p(inv_std), _p(dx), T, B, H),
             "batchnorm_bwd")


def batchnorm_fwd_dp(x, y, xhat, inv_std, group, scratch, eps=1e-3):
    """Batch norm whose batch axis spans the ranks of `group` (dataparallel.Group): moments over the GLOBAL batch.
    scratch: float32 [2, T, H] device buffer."""
    _chk_f32(x, y, xhat, inv_std, scratch)
    T, B, H = x.shape
    lib, n = _l.load(), B * group.world
    gsum, gsq = scratch[0], scratch[1]
    _l.check(lib.amdspeech_batchnorm_sum(_stream(), _p(x), _p(None), n, _p(gsum), T, B, H), "batchnorm_sum")
    group.all_reduce_sum_(gsum)
    _l.check(lib.amdspeech_batchnorm_sum(_stream(), _p(x), _p(gsum), n, _p(gsq), T, B, H), "batchnorm_sum")
    group.all_reduce_sum_(gsq)
    _l.check(lib.amdspeech_batchnorm_apply(_stream(), _p(x), _p(gsum), _p(gsq), n, eps, _p(y), _p(xhat), _p(inv_std), T, B, H),
             "batchnorm_apply")


def batchnorm_bwd_dp(dy, xhat, inv_std, dx, group, scratch):
    _chk_f32(dy, xhat, inv_std, dx, scratch)
    T, B, H = dy.shape
    lib, n = _l.load(), B * group.world
    sums = scratch.view(-1)[:2 * T * H]
    _l.check(lib.amdspeech_batchnorm_bwd_sums(_stream(), _p(dy), _p(xhat), _p(sums), T, B, H), "batchnorm_bwd_sums")
    group.all_reduce_sum_(sums)
    _l.check(lib.amdspeech_batchnorm_bwd_apply(_stream(), _p(dy), _p(xhat), _p(inv_std), _p(sums), n, _p(dx), T, B, H),
             "batchnorm_bwd_apply")


# -------------------------------------------------------------------------- LSTM
class _StackWorkspace(object):
    """What LstmWorkspace and BidirWorkspace share: the device allocation of one (T,B,H,L) descriptor, or a view of a longer one's
    (prefix()), and its named regions as tensor views (no copies).  A subclass names its library entry points (_BYTES, _PTR) and
    its messages (_NAME, _TOO_SMALL)."""

    def __init__(self, T, B, H, L, keep_in, keep_out, seed, device, precision, _share):
        self.lib = _l.load()
        self.desc = _l.LstmDesc(T, B, H, L, keep_in, keep_out, seed, int(precision))
        nbytes = getattr(self.lib, self._BYTES)(C.byref(self.desc))
        if nbytes == 0:
            raise _l.AmdSpeechError(self._NAME + ": " + self.lib.amdspeech_last_error().decode())
        self.T, self.B, self.H, self.L = T, B, H, L
        if _share is None:
            self.buf = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
        else:
            # (the owner's byte count covers every shorter run length of its shape; a view that does not fit would make the kernels
            #  write past the allocation -- an error in every build, not an assert)
            if _share.numel() * 4 < nbytes:
                raise _l.AmdSpeechError(self._TOO_SMALL % (T, nbytes, _share.numel() * 4))
            self.buf = _share
        if self.buf.data_ptr() % 256 != 0:
            raise _l.AmdSpeechError(self._NAME + ": allocation not 256-byte aligned")
        self._prefixes = {}
        self._root = self           # the owner of the allocation (prefix() views share it)

    def prefix(self, T_run):
        """The same allocation laid out for a shorter sequence (the layout is a pure function of the
        descriptor, and everything is time-major, so a batch whose longest utterance has T_run < T frames
        runs T_run + L - 1 diagonals instead of T + L - 1 -- what tf.nn.dynamic_rnn's while-loop does with
        max(sequence_length), reference models/AcousticModel.py:276-278)."""
        if T_run >= self.T:
            return self
        ws = self._prefixes.get(T_run)
        if ws is None:
            if len(self._prefixes) > 64:
                self._prefixes.clear()
            ws = type(self)(T_run, self.B, self.H, self.L, device=self.buf.device, precision=self.desc.precision, _share=self.buf)
            ws._root = self
            self._prefixes[T_run] = ws
        return ws

    def _offset(self, which):
        p = getattr(self.lib, self._PTR)(C.byref(self.desc), _p(self.buf), which)
        if not p:
            raise _l.AmdSpeechError(self._PTR[len("amdspeech_"):] + " failed")
        return (p - self.buf.data_ptr()) // 4

    def _view(self, which, shape):
        off = self._offset(which)
        n = 1
        for s in shape:
            n *= s
        return self.buf[off:off + n].view(*shape)

    def set_dropout(self, keep_in, keep_out, seed):
        self.desc.keep_in, self.desc.keep_out, self.desc.seed = keep_in, keep_out, seed


class LstmWorkspace(_StackWorkspace):
    """Owns the device workspace of one (T,B,H,L) LSTM stack and exposes the
    named regions as tensor views (no copies)."""
    _NAME, _BYTES, _PTR = "lstm workspace", "amdspeech_lstm_workspace_bytes", "amdspeech_lstm_ws_ptr"
    _TOO_SMALL = "lstm workspace: the layout for T = %d needs %d bytes, the shared allocation has %d"

    def __init__(self, T, B, H, L, keep_in=1.0, keep_out=1.0, seed=0, device="cuda", precision=0, _share=None):
        _StackWorkspace.__init__(self, T, B, H, L, keep_in, keep_out, seed, device, precision, _share)
        self.z0 = self._view(_l.WS_Z0, (T, B, H))
        self.ztop = self._view(_l.WS_ZTOP, (T, B, H))
        self.dztop = self._view(_l.WS_DZTOP, (T, B, H))
        self.dz0 = self._view(_l.WS_DZ0, (T, B, H))
        self._armed = None          # (root only) {"fwd": (T, precision) | None, "bwd": ...}: layouts whose hand-off panels are prepared
        self._ever_armed = False    # (root only) the library keeps side-stream state (events) for this allocation
        self._fwd_seen = False      # (root only) lstm_fwd has run on this allocation: the next one may say AMDSPEECH_LSTM_SAME_WS
        self._lib_state = False     # (root only) some lstm call has run on it: the library may hold events for the allocation (released in __del__)

    def __del__(self):
        # the library's side stream may still be filling hand-off panels of this allocation (AMDSPEECH_LSTM_ARM_NEXT): order the
        # current stream behind that work before torch's caching allocator may hand the memory to someone else
        try:
            # (whenever it has EVER been armed: an eval forward in between clears `_armed`, the library's entry for the allocation
            #  -- its events, a possibly pending fill -- stays until released)
            if self._root is self and (self._ever_armed or self._fwd_seen or self._lib_state) and torch.cuda.is_available():
                self.lib.amdspeech_lstm_workspace_release(_stream(), _p(self.buf))
        except Exception:      # interpreter shutdown: nothing left to protect
            pass

    def final_state(self):
        """(h [L,B,H], c [L,B,H]) views of the state after the last frame."""
        T, B, H, L = self.T, self.B, self.H, self.L
        stride = (T + 1) * B * H
        oh, oc = self._offset(_l.WS_HFINAL), self._offset(_l.WS_CFINAL)
        h = torch.as_strided(self.buf, (L, B, H), (stride, H, 1), oh)
        c = torch.as_strided(self.buf, (L, B, H), (stride, H, 1), oc)
        return h, c


_ARM = os.environ.get("AMDSPEECH_ARM", "1") != "0"      # 0: every call fills its own hand-off panels


class CtcHead(object):
    """The CTC head fused into the whole-sequence LSTM kernels (amdspeech.h: amdspeech_ctc_head): output Linear + log-softmax +
    alpha follow the forward recurrence, beta + gradient + dlogits . W_o^T run ahead of the backward recurrence -- nothing of the
    CTC stage is left between the two launches.  Holds the tensors the two calls of a mini-batch share."""

    def __init__(self, w_out, b_out, logits, dense_labels, loss, dlogits, ctc_ws):
        _chk_f32(w_out, b_out, logits, loss, dlogits)
        _chk_i32(dense_labels)
        T, B, C_ = logits.shape
        if ctc_ws.shape[0] < T or tuple(ctc_ws.shape[1:]) != (B, C_, dense_labels.shape[1]):      # (a prefix of the frames it was sized for is fine)
            raise ValueError("CtcHead: the CTC workspace was sized for %r, the logits are %r with U = %d"
                             % (ctc_ws.shape, (T, B, C_), dense_labels.shape[1]))
        self.keep = (w_out, b_out, logits, dense_labels, loss, dlogits, ctc_ws)
        self.c = _l.CtcHead(_p(w_out).value, _p(b_out).value, _p(logits).value, _p(dense_labels).value, _p(loss).value,
                            _p(dlogits).value if dlogits is not None else None, _p(ctc_ws.buf).value, C_, dense_labels.shape[1])


def lstm_ctc_fusable(ws, C_, U, per_diagonal=False):
    """Whether lstm_fwd / lstm_bwd on this workspace layout take a CtcHead (amdspeech_lstm_ctc_fusable)."""
    if per_diagonal:
        return False
    return bool(ws.lib.amdspeech_lstm_ctc_fusable(C.byref(ws.desc), int(C_), int(U)))


def _plan_desc(ws, per_diagonal):
    """A copy of the workspace's descriptor with the per-diagonal (per-frame) request as its only flag: what the plan queries read,
    so that they leave ws.desc alone."""
    d = ws.desc
    return _l.LstmDesc(d.T, d.B, d.H, d.L, d.keep_in, d.keep_out, d.seed, d.precision, _l.LSTM_PER_DIAGONAL if per_diagonal else 0)


def _head_c_u(head):
    """(C, U) of the CTC head a plan query is asked about: a CtcHead, or (C, U), or None (no head: (0, 0))."""
    if head is None:
        return 0, 0
    return (head.c.C, head.c.U) if isinstance(head, CtcHead) else (int(head[0]), int(head[1]))


def lstm_plan(ws, head=None, per_diagonal=False):
    """The kernel path lstm_fwd / lstm_bwd on this workspace layout take (amdspeech.h: amdspeech_lstm_plan), as a dict of ints with
    "fwd_path" / "bwd_path" as names ("flow", "big1", "big", "hoist", "diag", "diag_bf3").  head: a CtcHead, or (C, U), or None.
    Read-only: nothing is launched and the workspace's state is left alone."""
    c_u, d = _head_c_u(head), _plan_desc(ws, per_diagonal)
    info = _l.LstmPlanInfo()
    _l.check(ws.lib.amdspeech_lstm_plan(C.byref(d), c_u[0], c_u[1], C.byref(info)), "lstm_plan")
    out = _plan_dict(info)
    out["fwd_path"], out["bwd_path"] = _l.LSTM_PATHS[out["fwd_path"]], _l.LSTM_PATHS[out["bwd_path"]]
    return out


def _plan_xw(entry, ws, head, per_diagonal):
    """One of the forward dataflow launch's x-worker plan numbers (amdspeech_<entry>: an int, negative for a bad descriptor)."""
    c_u, d = _head_c_u(head), _plan_desc(ws, per_diagonal)
    n = int(getattr(ws.lib, "amdspeech_" + entry)(C.byref(d), c_u[0], c_u[1]))
    if n < 0:
        raise ValueError(entry + ": bad descriptor")
    return n


def lstm_plan_xw_halves(ws, head=None, per_diagonal=False):
    """The x-product workers' share of the forward dataflow launch in HALF K blocks per recurrence wave (amdspeech.h:
    amdspeech_lstm_plan_xw_halves): 0 none, 2 one block, 3 a block and a half (half roles).  Read-only, like lstm_plan."""
    return _plan_xw("lstm_plan_xw_halves", ws, head, per_diagonal)


def lstm_plan_xw_ksteps(ws, head=None, per_diagonal=False):
    """How many of the four k-steps of the K block below theirs the half roles of the forward dataflow launch take as well
    (amdspeech.h: amdspeech_lstm_plan_xw_ksteps); 0: none.  Read-only, like lstm_plan."""
    return _plan_xw("lstm_plan_xw_ksteps", ws, head, per_diagonal)


def lstm_fwd(ws, kernels, kernel_stride, biases, bias_stride, lengths, h0=None, c0=None, training=False, per_diagonal=False, head=None):
    """kernels/biases: tensors whose data_ptr is layer 0's K / bias; strides in elements.
    training: lstm_bwd on the same workspace follows; the call then prepares that call's hand-off panels and the next forward
    call's (the other of the workspace's two sets) beside its kernel (amdspeech.h: AMDSPEECH_LSTM_ARM_NEXT), and the next calls
    of the same layout skip their fills.
"""
    _chk_i32(lengths)
    _chk_f32(h0, c0)
    root, key = ws._root, (ws.T, int(ws.desc.precision))
    if per_diagonal:                # the re-run of a mini-batch whose dataflow launch timed out (amdspeech.h): nothing is armed
        root._armed, training = None, False
    armed = _ARM and root._armed is not None and root._armed["fwd"] == key
    root._armed = None              # whatever runs now, the panels are in use
    inject, root._inject_timeout = getattr(root, "_inject_timeout", 0), 0       # (tests: ONE dataflow launch that gives up)
    # (SAME_WS: every view of one allocation shares B / H / L / precision, and nothing but the lstm calls writes into it)
    ws.desc.flags = ((_l.LSTM_ARMED if armed else 0) | (_l.LSTM_ARM_NEXT if (training and _ARM) else 0) |
                     (_l.LSTM_SAME_WS if (root._fwd_seen and _ARM) else 0) | (_l.LSTM_PER_DIAGONAL if per_diagonal else 0) |
                     (_l.LSTM_INJECT_TIMEOUT if inject else 0))
    root._fwd_seen = False          # (a call that raises leaves the history in an unknown state)
    try:
        if head is None:
            _l.check(ws.lib.amdspeech_lstm_fwd(_stream(), C.byref(ws.desc), _p(ws.buf), _p(kernels), kernel_stride,
                                               _p(biases), bias_stride, _p(lengths), _p(h0), _p(c0)), "lstm_fwd")
        else:
            _l.check(ws.lib.amdspeech_lstm_fwd_ctc(_stream(), C.byref(ws.desc), _p(ws.buf), _p(kernels), kernel_stride,
                                                   _p(biases), bias_stride, _p(lengths), _p(h0), _p(c0), C.byref(head.c)), "lstm_fwd_ctc")
        # (a launch-per-diagonal run at a shorter prefix writes over x-product history frames the NEXT whole-sequence launch would
        #  trust under SAME_WS: it leaves the history "unknown" -- the library keeps state for the allocation all the same)
        root._fwd_seen = not per_diagonal
        root._lib_state = True
    finally:
        ws.desc.flags = 0
    if training and _ARM:
        root._armed = {"fwd": key, "bwd": key}
        root._ever_armed = True


def lstm_pair_fusable(ws):
    """The layers of two stacks of this shape run side by side (amdspeech.h: amdspeech_lstm_pair_fusable)."""
    ws.desc.flags = 0
    return bool(ws.lib.amdspeech_lstm_pair_fusable(C.byref(ws.desc)))


def lstm_fwd_pair(ws_a, kernels_a, biases_a, ws_b, kernels_b, biases_b, kernel_stride, bias_stride, lengths, h0=None, c0=None):
    """Two stacks of one shape over one batch (a bidirectional model's two directions; h0 / c0: stack A's initial state).  The results
    of lstm_fwd(ws_a ...) followed by lstm_fwd(ws_b ...); where the library can, the two stacks' layers run side by side in one
    launch each (amdspeech.h: amdspeech_lstm_fwd_pair).  Nothing is armed: shapes that take this path have no hand-off panels."""
    _chk_i32(lengths)
    _chk_f32(h0, c0)
    for ws in (ws_a, ws_b):
        ws._root._armed, ws._root._fwd_seen, ws._root._lib_state = None, False, True
        ws.desc.flags = 0
    _l.check(ws_a.lib.amdspeech_lstm_fwd_pair(_stream(), C.byref(ws_a.desc), _p(ws_a.buf), _p(kernels_a), _p(biases_a),
                                              C.byref(ws_b.desc), _p(ws_b.buf), _p(kernels_b), _p(biases_b),
                                              kernel_stride, bias_stride, _p(lengths), _p(h0), _p(c0)), "lstm_fwd_pair")


def lstm_status(ws):
    """Synchronous check that no bounded wait of the persistent kernels timed out."""
    try:
        _l.check(ws.lib.amdspeech_lstm_status(C.byref(ws.desc), _p(ws.buf)), "lstm_status")
    except _l.AmdSpeechError:
        ws._root._armed = None          # (nothing of that launch's hand-off state is to be trusted: the next calls fill for themselves)
        ws._root._fwd_seen = False
        raise


def lstm_beside_forward(ws, stream):
    """Orders `stream` (a torch.cuda.Stream) behind the point just in front of the last lstm_fwd launch on `ws` and returns the
    number of XCDs that launch leaves idle (0: not a whole-sequence dataflow launch -- nothing is ordered).  Work-queue kernels
    enqueued on `stream` afterwards do their work beside the forward recurrence (amdspeech.h: amdspeech_lstm_beside_forward)."""
    rc = _l.load().amdspeech_lstm_beside_forward(C.c_void_p(stream.cuda_stream), _p(ws._root.buf))
    if rc < 0:
        _l.check(rc, "lstm_beside_forward")
    return rc


def lstm_beside_tail(ws, stream):
    """Orders `stream` behind the last lstm_bwd's whole-sequence kernel on `ws`, in FRONT of the weight-gradient launches that follow
    it on the caller's stream (amdspeech.h: amdspeech_lstm_beside_tail).  Returns 0 (nothing ordered) or flags: 1 ordered, 2 dZ_0 is
    complete at that point."""
    rc = _l.load().amdspeech_lstm_beside_tail(C.c_void_p(stream.cuda_stream), _p(ws._root.buf))
    if rc < 0:
        _l.check(rc, "lstm_beside_tail")
    return rc


def lstm_bwd(ws, kernels, kernel_stride, dkernels, dbiases, bias_stride, lengths, per_diagonal=False, head=None):
    _chk_i32(lengths)
    root, key = ws._root, (ws.T, int(ws.desc.precision))
    armed = root._armed is not None and root._armed["bwd"] == key and not per_diagonal
    if root._armed is not None:
        root._armed["bwd"] = None       # (used once; the forward half stays valid for the next lstm_fwd)
    root._lib_state = True
    inject, root._inject_timeout_bwd = getattr(root, "_inject_timeout_bwd", 0), 0      # (tests: ONE backward dataflow launch that gives up)
    ws.desc.flags = ((_l.LSTM_ARMED if armed else 0) | (_l.LSTM_PER_DIAGONAL if per_diagonal else 0) |
                     (_l.LSTM_INJECT_TIMEOUT if inject else 0))
    try:
        if head is None:
            _l.check(ws.lib.amdspeech_lstm_bwd(_stream(), C.byref(ws.desc), _p(ws.buf), _p(kernels), kernel_stride,
                                               _p(dkernels), _p(dbiases), bias_stride, _p(lengths)), "lstm_bwd")
        else:
            _l.check(ws.lib.amdspeech_lstm_bwd_ctc(_stream(), C.byref(ws.desc), _p(ws.buf), _p(kernels), kernel_stride,
                                                   _p(dkernels), _p(dbiases), bias_stride, _p(lengths), C.byref(head.c)), "lstm_bwd_ctc")
    finally:
        ws.desc.flags = 0


def lstm_bwd_pair(ws_a, kernels_a, dkernels_a, dbiases_a, ws_b, kernels_b, dkernels_b, dbiases_b, kernel_stride, bias_stride, lengths):
    """The backward passes of the two stacks of lstm_fwd_pair (dztop of either workspace filled): the results of two lstm_bwd calls,
    side by side where the library can (amdspeech.h: amdspeech_lstm_bwd_pair)."""
    _chk_i32(lengths)
    for ws in (ws_a, ws_b):
        if ws._root._armed is not None:
            ws._root._armed["bwd"] = None
        ws._root._lib_state = True
        ws.desc.flags = 0
    _l.check(ws_a.lib.amdspeech_lstm_bwd_pair(_stream(), C.byref(ws_a.desc), _p(ws_a.buf), _p(kernels_a), _p(dkernels_a), _p(dbiases_a),
                                              C.byref(ws_b.desc), _p(ws_b.buf), _p(kernels_b), _p(dkernels_b), _p(dbiases_b),
                                              kernel_stride, bias_stride, _p(lengths)), "lstm_bwd_pair")


def lstm_dropout_multipliers(ws, which, layer):
    """[T,B,H] inverted-dropout multipliers (mask / keep) the LSTM calls on `ws` apply with its current keep_in / keep_out /
    seed: which = "in" / "out" mask of `layer` (DropoutWrapper, reference :227-233)."""
    out = torch.empty(ws.T, ws.B, ws.H, device=ws.buf.device, dtype=torch.float32)
    _l.check(ws.lib.amdspeech_lstm_dropout_multipliers(_stream(), C.byref(ws.desc), {"in": 0, "out": 1}[which], int(layer),
                                                       _p(out)), "lstm_dropout_multipliers")
    return out


class BidirWorkspace(_StackWorkspace):
    """Workspace of a layer-wise bidirectional stack (amdspeech.h: amdspeech_lstm_bidir_*): named regions as tensor views.
    precision: 0 = exact f32, 1 = bf16x3 (the recurrent and batched products as three bf16 MFMAs per product)."""
    _NAME, _BYTES, _PTR = "lstm bidir workspace", "amdspeech_lstm_bidir_workspace_bytes", "amdspeech_lstm_bidir_ws_ptr"
    _TOO_SMALL = "lstm bidir workspace: T = %d needs %d bytes, the shared allocation has %d"

    def __init__(self, T, B, H, L, device="cuda", precision=0, _share=None):
        _StackWorkspace.__init__(self, T, B, H, L, 1.0, 1.0, 0, device, precision, _share)
        self.precision = precision
        self.z0 = self._view(_l.BIDIR_WS_Z0, (T, B, H))
        self.ytop_fw = self._view(_l.BIDIR_WS_YTOP_FW, (T, B, H))
        self.ytop_bw = self._view(_l.BIDIR_WS_YTOP_BW, (T, B, H))
        self.dytop_fw = self._view(_l.BIDIR_WS_DYTOP_FW, (T, B, H))
        self.dytop_bw = self._view(_l.BIDIR_WS_DYTOP_BW, (T, B, H))
        self.dz0 = self._view(_l.BIDIR_WS_DZ0, (T, B, H))

    def path(self):
        """2: both directions of a layer in one persistent launch, 1: one persistent launch per direction, 0: one launch per frame."""
        return lstm_bidir_plan(self)["path"]

    def final_state(self):
        """(h [L,B,H], c [L,B,H]) of the forward cells after the last frame."""
        stride = self.lib.amdspeech_lstm_bidir_layer_stride(C.byref(self.desc))
        B, H, L = self.B, self.H, self.L
        h = torch.as_strided(self.buf, (L, B, H), (stride, H, 1), self._offset(_l.BIDIR_WS_HFINAL))
        c = torch.as_strided(self.buf, (L, B, H), (stride, H, 1), self._offset(_l.BIDIR_WS_CFINAL))
        return h, c

    def layer_outputs(self):
        """(y_fw [L,T,B,H], y_bw [L,T,B,H]): read-only views of every layer's outputs in forward time; the top layer's are
        ytop_fw / ytop_bw, layer l lies L - 1 - l layer strides below them (amdspeech_lstm_bidir_layer_stride)."""
        stride = self.lib.amdspeech_lstm_bidir_layer_stride(C.byref(self.desc))
        T, B, H, L = self.T, self.B, self.H, self.L
        return tuple(torch.as_strided(self.buf, (L, T, B, H), (stride, B * H, H, 1), self._offset(which) - (L - 1) * stride)
                     for which in (_l.BIDIR_WS_YTOP_FW, _l.BIDIR_WS_YTOP_BW))


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def lstm_bidir_plan(ws, per_frame=False):
    """What lstm_bidir_fwd / lstm_bidir_bwd on this workspace layout launch for the recurrence (amdspeech.h: amdspeech_lstm_bidir_plan),
    as a dict of ints: path, cus, and kpw / waves / groups / wgs / lds of the forward (fwd_*) and backward (bwd_*) kernel.
    Read-only: nothing is launched and ws.desc.flags is left alone."""
    d = _plan_desc(ws, per_frame)
    info = _l.LstmBidirPlanInfo()
    _l.check(ws.lib.amdspeech_lstm_bidir_plan(C.byref(d), C.byref(info)), "lstm_bidir_plan")
    return _plan_dict(info)


def lstm_bidir_fwd(ws, kernels, biases, lengths, h0=None, c0=None, per_frame=False, inject_timeout=False):
    """Layer-wise bidirectional forward (amdspeech_lstm_bidir_fwd): kernels / biases = the 2L cell tensors, forward cells first.
    Reads ws.z0, writes ws.ytop_fw / ws.ytop_bw (forward time)."""
    _chk_i32(lengths)
    _chk_f32(*kernels, *biases)
    ws.desc.flags = (_l.LSTM_PER_DIAGONAL if per_frame else 0) | (_l.LSTM_INJECT_TIMEOUT if inject_timeout else 0)
    try:
        _l.check(ws.lib.amdspeech_lstm_bidir_fwd(_stream(), C.byref(ws.desc), _p(ws.buf), _ptr_array(kernels), _ptr_array(biases),
                                                 _p(lengths), _p(h0), _p(c0)), "lstm_bidir_fwd")
    finally:
        ws.desc.flags = 0


def lstm_bidir_bwd(ws, kernels, dkernels, dbiases, lengths, per_frame=False, inject_timeout=False):
    """Its backward pass: reads ws.dytop_fw / ws.dytop_bw, writes ws.dz0, accumulates into dkernels / dbiases."""
    _chk_i32(lengths)
    ws.desc.flags = (_l.LSTM_PER_DIAGONAL if per_frame else 0) | (_l.LSTM_INJECT_TIMEOUT if inject_timeout else 0)
    try:
        _l.check(ws.lib.amdspeech_lstm_bidir_bwd(_stream(), C.byref(ws.desc), _p(ws.buf), _ptr_array(kernels), _ptr_array(dkernels),
                                                 _ptr_array(dbiases), _p(lengths)), "lstm_bidir_bwd")
    finally:
        ws.desc.flags = 0


def lstm_bidir_status(ws):
    """Synchronous check that no bounded wait of the persistent per-layer kernels timed out (DataflowTimeout if one did)."""
    _l.check(ws.lib.amdspeech_lstm_bidir_status(C.byref(ws.desc), _p(ws.buf)), "lstm_bidir_status")


def lstm_bidir_dropout_multipliers(ws, direction, which, layer):
    """The multipliers one cell applies (step order): direction "fw" / "bw", which "in" ([T,B,W], W = H at layer 0, 2H above) or
    "out" ([T,B,H])."""
    W = ws.H if (which == "out" or layer == 0) else 2 * ws.H
    out = torch.empty(ws.T, ws.B, W, device=ws.buf.device, dtype=torch.float32)
    _l.check(ws.lib.amdspeech_lstm_bidir_dropout_multipliers(_stream(), C.byref(ws.desc), {"fw": 0, "bw": 1}[direction],
                                                             {"in": 0, "out": 1}[which], int(layer), _p(out)),
             "lstm_bidir_dropout_multipliers")
    return out


def reverse_sequences(x, lengths, out=None, accumulate=False):
    """Time-major [T,B,H]: out[t,b] = x[len_b-1-t, b] for t < len_b, 0 beyond (tf.reverse_sequence; self-adjoint)."""
    _chk_f32(x, out)
    _chk_i32(lengths)
    T, B, H = x.shape
    if out is None:
        out = torch.empty_like(x)
    _l.check(_l.load().amdspeech_reverse_sequences(_stream(), _p(x), _p(out), _p(lengths), T, B, H, int(bool(accumulate))),
             "reverse_sequences")
    return out


# --------------------------------------------------------------------------- CTC
class CtcWorkspace(object):
    def __init__(self, T, B, C_, U, device="cuda"):
        self.lib = _l.load()
        n = self.lib.amdspeech_ctc_workspace_bytes(T, B, C_, U)
        if n == 0:
            raise _l.AmdSpeechError("ctc workspace: bad shape")
        self.shape = (T, B, C_, U)
        self.buf = torch.empty(n, device=device, dtype=torch.uint8)
        self.greedy_ws = torch.empty(T * B, device=device, dtype=torch.int32)


def ctc_plan(T, B, C_, U):
    """The recursion kernel ctc_loss_fwd_bwd takes for a shape (amdspeech.h: amdspeech_ctc_plan), as a dict of ints with "kernel" as a
    name ("wave", "shift", "pair", "edge").  Read-only: nothing is launched.  A shape the call refuses raises here too."""
    info = _l.CtcPlanInfo()
    _l.check(_l.load().amdspeech_ctc_plan(int(T), int(B), int(C_), int(U), C.byref(info)), "ctc_plan")
    out = _plan_dict(info)
    out["kernel"] = _l.CTC_KERNELS[out["kernel"]]
    return out


def ctc_loss_fwd_bwd(logits, dense_labels, lengths, ws=None, loss=None, dlogits=None, stage=0):
    """logits [T,B,C]; dense_labels int32 [B,U] (0-padded, reference labels_ph);
    returns (loss [B], dlogits [T,B,C]).  stage 1 / 2: the two halves of the call (amdspeech.h), same arguments."""
    _chk_f32(logits, loss, dlogits)
    _chk_i32(dense_labels, lengths)
    T, B, C_ = logits.shape
    U = dense_labels.shape[1]
    if ws is None or ws.shape[1:] != (B, C_, U) or ws.shape[0] < T:     # a longer-T workspace serves a prefix
        ws = CtcWorkspace(T, B, C_, U, logits.device)
    if loss is None:
        loss = torch.empty(B, device=logits.device, dtype=torch.float32)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    _l.check(ws.lib.amdspeech_ctc_loss_fwd_bwd_staged(_stream(), _p(logits), _p(dense_labels), _p(lengths), T, B, C_, U,
                                                      _p(loss), _p(dlogits), _p(ws.buf), int(stage)), "ctc_loss_fwd_bwd")
    return loss, dlogits


class CtcAlignWorkspace(object):
    """The aligner's own workspace (amdspeech.h: amdspeech_ctc_align_workspace_bytes): log p, extended targets, back-pointers."""

    def __init__(self, T, B, C_, U, device="cuda"):
        self.lib = _l.load()
        n = self.lib.amdspeech_ctc_align_workspace_bytes(T, B, C_, U)
        if n == 0:
            raise _l.AmdSpeechError("ctc align workspace: bad shape")
        self.shape = (T, B, C_, U)
        self.buf = torch.empty(n, device=device, dtype=torch.uint8)


class CtcAlignment(object):
    """What ctc_align returns, all device tensors (amdspeech.h: amdspeech_ctc_align): frame_label [B,T], frame_state [B,T],
    spans [B,U,2] int32; score [B], confidence [B,U] float32."""
    __slots__ = ("frame_label", "frame_state", "spans", "score", "confidence")

    def __init__(self, frame_label, frame_state, spans, score, confidence):
        self.frame_label, self.frame_state, self.spans, self.score, self.confidence = frame_label, frame_state, spans, score, confidence


def ctc_align_plan(T, B, C_, U):
    """The recursion kernel ctc_align takes for a shape (amdspeech.h: amdspeech_ctc_align_plan), as ctc_plan reports the loss's."""
    info = _l.CtcPlanInfo()
    _l.check(_l.load().amdspeech_ctc_align_plan(int(T), int(B), int(C_), int(U), C.byref(info)), "ctc_align_plan")
    out = _plan_dict(info)
    out["kernel"] = _l.CTC_KERNELS[out["kernel"]]
    return out


def ctc_align(logits, dense_labels, lengths, ws=None):
    """The best CTC alignment of the transcripts to the frames: logits [T,B,C]; dense_labels int32 [B,U] (0-padded, as
    ctc_loss_fwd_bwd takes them); lengths int32 [B].  Returns a CtcAlignment."""
    _chk_f32(logits)
    _chk_i32(dense_labels, lengths)
    T, B, C_ = logits.shape
    U = dense_labels.shape[1]
    if ws is None or ws.shape != (T, B, C_, U):      # (the back-pointer rows are laid out by T: no prefix use)
        ws = CtcAlignWorkspace(T, B, C_, U, logits.device)
    dev = logits.device
    out = CtcAlignment(torch.empty(B, T, device=dev, dtype=torch.int32), torch.empty(B, T, device=dev, dtype=torch.int32),
                       torch.empty(B, U, 2, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.float32),
                       torch.empty(B, U, device=dev, dtype=torch.float32))
    _l.check(ws.lib.amdspeech_ctc_align(_stream(), _p(logits), _p(dense_labels), _p(lengths), T, B, C_, U, _p(out.frame_label),
                                        _p(out.frame_state), _p(out.spans), _p(out.score), _p(out.confidence), _p(ws.buf)), "ctc_align")
    return out


def ctc_greedy_decode(logits, lengths, ws=None):
    """Returns (ids int32 [B,T] padded with C, out_len int32 [B])."""
    _chk_f32(logits)
    _chk_i32(lengths)
    T, B, C_ = logits.shape
    scratch = ws.greedy_ws if ws is not None and ws.shape[:2] == (T, B) else \
        torch.empty(T * B, device=logits.device, dtype=torch.int32)
    ids = torch.empty(B, T, device=logits.device, dtype=torch.int32)
    out_len = torch.empty(B, device=logits.device, dtype=torch.int32)
    _l.check(_l.load().amdspeech_ctc_greedy_decode(_stream(), _p(logits), _p(lengths), T, B, C_, _p(ids),
                                                   _p(out_len), _p(scratch)), "ctc_greedy_decode")
    return ids, out_len


def merge_repeated(ids, lens, pad):
    """In place on the device: collapse consecutive duplicate labels of each row."""
    _chk_i32(ids, lens)
    B, T = ids.shape
    _l.check(_l.load().amdspeech_merge_repeated(_stream(), _p(ids), _p(lens), T, B, int(pad)), "merge_repeated")
    return ids, lens


def edit_distance(a, a_len, b, b_len):
    """Levenshtein distance per row pair, int32 [n] on the device."""
    _chk_i32(a, a_len, b, b_len)
    n = a.shape[0]
    out = torch.empty(n, device=a.device, dtype=torch.int32)
    _l.check(_l.load().amdspeech_edit_distance(_stream(), _p(a), _p(a_len), a.shape[1], _p(b), _p(b_len),
                                               b.shape[1], n, _p(out)), "edit_distance")
    return out


def edit_distance_host(a, a_len, b, b_len):
    """Levenshtein distance per row pair on the HOST (numpy int32 in, int32 [n] out): for predictions decoded on the host."""
    import numpy as np
    a = np.ascontiguousarray(a, np.int32); b = np.ascontiguousarray(b, np.int32)
    a_len = np.ascontiguousarray(a_len, np.int32); b_len = np.ascontiguousarray(b_len, np.int32)
    n = a.shape[0]
    out = np.empty(n, np.int32)
    _l.check(_l.load().amdspeech_edit_distance_host(a.ctypes.data_as(C.c_void_p), a_len.ctypes.data_as(C.c_void_p), a.shape[1],
                                                    b.ctypes.data_as(C.c_void_p), b_len.ctypes.data_as(C.c_void_p), b.shape[1], n,
                                                    out.ctypes.data_as(C.c_void_p)), "edit_distance_host")
    return out


def ctc_beam_search(logits, lengths, beam_width=100, merge_repeated=True, max_threads=0):
    """Host-side prefix beam search (evaluation path).  logits: [T,B,C] tensor or array (copied to the
    host), lengths: ints.  Returns (ids int32 [B,T] numpy padded with C, out_len [B], log_prob [B]).
    max_threads > 0 caps the decode threads of the call (default: one per utterance)."""
    import numpy as np
    host = logits.detach().cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits)
    host = np.ascontiguousarray(host, np.float32)
    T, B, C_ = host.shape
    lens = np.ascontiguousarray(lengths.cpu().numpy() if torch.is_tensor(lengths) else lengths, np.int32)
    ids = np.empty((B, T), np.int32)
    out_len = np.empty(B, np.int32)
    logp = np.empty(B, np.float32)
    _l.check(_l.load().amdspeech_ctc_beam_search_host_mt(
        host.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), T, B, C_, int(beam_width),
        int(bool(merge_repeated)), ids.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p),
        logp.ctypes.data_as(C.c_void_p), int(max_threads)), "ctc_beam_search_host")
    return ids, out_len, logp


def ctc_beam_search_nbest(logits, lengths, n_best, beam_width=100, merge_repeated=True, max_threads=0):
    """The n-best list of the same search (amdspeech.h: amdspeech_ctc_beam_search_host_nbest): the first n_best entries of the
    final beam, best first; entry 0 is ctc_beam_search's answer.  Returns numpy (ids int32 [B,n_best,T] padded with C,
    out_len [B,n_best], log_prob float32 [B,n_best] with -inf in unused slots, n_found [B])."""
    import numpy as np
    host = logits.detach().cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits)
    host = np.ascontiguousarray(host, np.float32)
    T, B, C_ = host.shape
    n_best = int(n_best)
    lens = np.ascontiguousarray(lengths.cpu().numpy() if torch.is_tensor(lengths) else lengths, np.int32)
    ids = np.empty((B, max(n_best, 0), T), np.int32)
    out_len = np.empty((B, max(n_best, 0)), np.int32)
    logp = np.empty((B, max(n_best, 0)), np.float32)
    n_found = np.empty(B, np.int32)
    _l.check(_l.load().amdspeech_ctc_beam_search_host_nbest(
        host.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), T, B, C_, int(beam_width),
        int(bool(merge_repeated)), n_best, ids.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p),
        logp.ctypes.data_as(C.c_void_p), n_found.ctypes.data_as(C.c_void_p), int(max_threads)), "ctc_beam_search_host_nbest")
    return ids, out_len, logp, n_found


def ctc_blank_skip_plan(T, B, C_):
    """The kernels ctc_blank_skip takes for a shape (amdspeech.h: amdspeech_ctc_blank_skip_plan), as a dict of ints with "kernel" as
    a name ("wave", "block"); c_min .. c_max is the range of C on the same row kernel, t_chunk the frames per step of the
    per-utterance scan.  Read-only, no device needed; a shape the call refuses raises here too."""
    info = _l.BlankSkipPlanInfo()
    _l.check(_l.load().amdspeech_ctc_blank_skip_plan(int(T), int(B), int(C_), C.byref(info)), "ctc_blank_skip_plan")
    out = _plan_dict(info)
    out["kernel"] = _l.BLANK_SKIP_KERNELS[out["kernel"]]
    return out


_blank_skip_ws = {}


def ctc_blank_skip(logits, lengths, threshold, out=None, new_lengths=None, src_frame=None, blank_logp=None):
    """Blank-frame skipping in front of a beam decoder (amdspeech.h: amdspeech_ctc_blank_skip).  logits float32 [T,B,C] and lengths
    int32 [B] on the device; threshold: the blank probability in (0, 1] at and above which a frame is skippable (the library gets
    its log).  Of every run of skippable frames the first is kept.  Returns (compact [T,B,C]: the kept frames of every utterance
    moved to the front, zeros behind them; new_lengths int32 [B]; src_frame int32 [B,T]: the source frame of every kept one, -1
    behind them).  blank_logp: an optional float32 [T,B] that receives the blank log-posterior of every frame inside its row."""
    import math
    T, B, C_ = _chk_f32_3d("ctc_blank_skip", logits, "[T, B, C]")
    _chk_i32(lengths)
    _chk_f32(out, blank_logp)
    threshold = float(threshold)
    if not 0.0 < threshold <= 1.0:
        raise ValueError("ctc_blank_skip: threshold %r is not a probability in (0, 1]" % threshold)
    if lengths.numel() != B:
        raise ValueError("ctc_blank_skip: %d lengths for %d utterances" % (lengths.numel(), B))
    dev = logits.device
    if out is None:
        out = torch.empty_like(logits)
    if new_lengths is None:
        new_lengths = torch.empty(B, device=dev, dtype=torch.int32)
    if src_frame is None:
        src_frame = torch.empty(B, T, device=dev, dtype=torch.int32)
    _chk_i32(new_lengths, src_frame)
    if tuple(out.shape) != (T, B, C_) or new_lengths.numel() != B or tuple(src_frame.shape) != (B, T) \
            or (blank_logp is not None and tuple(blank_logp.shape) != (T, B)):
        raise ValueError("ctc_blank_skip: an output does not fit T = %d, B = %d, C = %d" % (T, B, C_))
    lib = _l.load()
    ws = _cached_ws(_blank_skip_ws, (T, B, C_, dev), lambda: max(int(lib.amdspeech_ctc_blank_skip_workspace_bytes(T, B, C_)), 16))
    _l.check(lib.amdspeech_ctc_blank_skip(_stream(), _p(logits), _p(lengths), T, B, C_, math.log(threshold), _p(out), _p(new_lengths),
                                          _p(src_frame), _p(blank_logp), _p(ws)), "ctc_blank_skip")
    return out, new_lengths, src_frame


# --------------------------------------------------------------------- optimiser
_optim_ws = {}


def clip_adam(params, grads, m, v, clip, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, norm_out=None):
    _chk_f32(params, grads, m, v)
    n = params.numel()
    key = params.device
    if key not in _optim_ws:
        _optim_ws[key] = torch.empty(_l.load().amdspeech_optim_workspace_bytes(n) // 4, device=params.device,
                                     dtype=torch.float32)
    if norm_out is None:
        norm_out = torch.empty(1, device=params.device, dtype=torch.float32)
    _l.check(_l.load().amdspeech_clip_adam(_stream(), _p(params), _p(grads), _p(m), _p(v), n, clip, lr_t, beta1,
                                           beta2, eps, _p(norm_out), _p(_optim_ws[key])), "clip_adam")
    return norm_out


# --------------------------------------------------------------------- front end
_frontend_ws = {}


def audio_probe(path):
    """(sample_rate, channels, frames) from the header of a WAVE / FLAC / NIST SPHERE file (host)."""
    sr, ch, fr = C.c_int(), C.c_int(), C.c_long()
    _l.check(_l.load().amdspeech_audio_probe(str(path).encode(), C.byref(sr), C.byref(ch), C.byref(fr)), "audio_probe")
    return sr.value, ch.value, fr.value


def audio_decode(path, verify=False):
    """Mono float32 numpy array in [-1, 1) and the file's sample rate (host; ctypes releases the GIL, so
    a thread pool decodes files in parallel).  verify: also check the FLAC STREAMINFO MD5."""
    import numpy as np
    lib = _l.load()
    enc = str(path).encode()
    sr, ch, fr = C.c_int(), C.c_int(), C.c_long()
    _l.check(lib.amdspeech_audio_probe(enc, C.byref(sr), C.byref(ch), C.byref(fr)), "audio_probe")
    out = np.empty(max(fr.value, 1), np.float32)
    got = C.c_long()
    _l.check(lib.amdspeech_audio_decode(enc, C.c_void_p(out.ctypes.data), out.size, C.byref(got), C.byref(sr),
                                        int(bool(verify))), "audio_decode")
    return out[:got.value], sr.value


def resample(pcm, n_samples, rate_in, rate_out):
    """pcm float32 [B, n_max] (device), n_samples python ints -> (out [B, out_max] device, new lengths):
    librosa.load's resampling step (resampy kaiser_best semantics), on the GPU: resample_rows with every row at 1000 permille."""
    return resample_rows(pcm, n_samples, [1000] * len(n_samples), rate_in, rate_out)


_resample_rows_ws = {}


def resample_rows_num_samples(n, rate_in, rate_out, speed_permille=1000):
    """Samples a row of n samples becomes: ceil(n * rate_out * 1000 / (rate_in * speed_permille)), exact integer arithmetic on the
    host (amdspeech.h: amdspeech_resample_rows_num_samples)."""
    got = _l.load().amdspeech_resample_rows_num_samples(int(n), int(rate_in), int(rate_out), int(speed_permille))
    if got < 0:
        _l.check(got, "resample_rows_num_samples")
    return got


def resample_rows_plan(n_samples, speed_permille, n_max, rate_in, rate_out, out_max=None):
    """The launch geometry of `resample_rows` for these rows (amdspeech.h: amdspeech_resample_rows_plan), as a dict of ints.
    out_max None: the longest output row, as resample_rows sizes it.  Read-only: nothing is launched, no device is needed.  What
    the call refuses raises here too."""
    B = len(n_samples)
    ns, pm = _c_ints(n_samples, B, "resample_rows_plan"), _c_ints(speed_permille, B, "resample_rows_plan")
    if out_max is None:
        out_max = max([resample_rows_num_samples(n, rate_in, rate_out, s) for n, s in zip(n_samples, speed_permille)] + [1])
    info = _l.ResampleRowsPlanInfo()
    _l.check(_l.load().amdspeech_resample_rows_plan(ns, pm, B, int(n_max), int(rate_in), int(rate_out), int(out_max), C.byref(info)),
             "resample_rows_plan")
    return _plan_dict(info)


def resample_rows(pcm, n_samples, speed_permille, rate_in, rate_out, out=None):
    """pcm float32 [B, n_max] (device), n_samples and speed_permille python ints per row -> (out [B, out_max] device, new lengths):
    every row resampled from rate_in * speed / 1000 to rate_out in ONE launch -- rate conversion and speed change together
    (amdspeech.h: amdspeech_resample_rows).  A row whose ratio is exactly 1 is copied bit for bit.  Every word of out is written;
    input words at or past a row's length are not read.  out: an [B, out_max] tensor to fill (out_max at least the longest row)."""
    _chk_f32(pcm, out)
    if pcm.dim() != 2:
        raise ValueError("resample_rows: expected [B, n_max], got %s" % (tuple(pcm.shape),))
    lib = _l.load()
    B, n_max = pcm.shape
    ns, pm = _c_ints(n_samples, B, "resample_rows"), _c_ints(speed_permille, B, "resample_rows")
    n_out = [resample_rows_num_samples(n, rate_in, rate_out, s) for n, s in zip(n_samples, speed_permille)]
    if out is None:
        out = torch.empty(B, max(max(n_out), 1), device=pcm.device, dtype=torch.float32)
    elif out.dim() != 2 or out.shape[0] != B or out.device != pcm.device:
        raise ValueError("resample_rows: out is %s on %s, expected [%d, out_max] beside pcm" % (tuple(out.shape), out.device, B))
    ws = _cached_ws(_resample_rows_ws, (B, pcm.device), lambda: lib.amdspeech_resample_rows_workspace_bytes(B))
    _l.check(lib.amdspeech_resample_rows(_stream(), _p(pcm), ns, pm, B, n_max, int(rate_in), int(rate_out), _p(out), out.shape[1],
                                         _p(ws)), "resample_rows")
    return out, n_out          # stream-ordered; lengths and speeds were kernel arguments, the cached workspace outlives the kernels


def speed_perturb_draw(seed, index, factors_permille):
    """The speed (permille) of utterance `index` under `seed`, one of factors_permille (1 .. 8 values in 500 .. 2000): SpecAugment's
    integer hash on the host (amdspeech.h: amdspeech_speed_perturb_draw)."""
    f = _c_ints(factors_permille, len(factors_permille), "speed_perturb_draw")
    got = _l.load().amdspeech_speed_perturb_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(index) & 0xFFFFFFFFFFFFFFFF, f, len(factors_permille))
    if got < 0:
        _l.check(got, "speed_perturb_draw")
    return got


# ------------------------------------------------ noise and reverberation augmentation
_augment_ws = {}


def _chk_rows(what, pcm, out=None):
    """pcm (and out) are contiguous float32 device tensors [B, n_max]; returns (B, n_max)."""
    _chk_f32(pcm, out)
    if pcm.dim() != 2:
        raise ValueError("%s: expected [B, n_max], got %s" % (what, tuple(pcm.shape)))
    if out is not None and (out.shape != pcm.shape or out.device != pcm.device):
        raise ValueError("%s: out is %s on %s, expected %s beside pcm" % (what, tuple(out.shape), out.device, tuple(pcm.shape)))
    return pcm.shape


def _chk_f64_vec(what, t, count, device):
    if not (torch.is_tensor(t) and t.dtype == torch.float64 and t.dim() == 1 and t.shape[0] == count and t.is_contiguous()
            and t.device == device):
        raise ValueError("%s: expected %d contiguous float64 values on %s" % (what, count, device))


def reverb_rows_plan(n_samples, n_max, rir_taps, rir_delay, taps_max, rir_index):
    """The launch geometry of `reverb_rows` for these rows (amdspeech.h: amdspeech_reverb_rows_plan), as a dict of ints.  Read-only:
    nothing is launched, no device is needed.  What the call refuses raises here too."""
    B, R = len(n_samples), len(rir_taps)
    info = _l.ReverbRowsPlanInfo()
    _l.check(_l.load().amdspeech_reverb_rows_plan(_c_ints(n_samples, B, "reverb_rows_plan"), B, int(n_max),
                                                  _c_ints(rir_taps, R, "reverb_rows_plan"), _c_ints(rir_delay, R, "reverb_rows_plan"), R,
                                                  int(taps_max), _c_ints(rir_index, B, "reverb_rows_plan"), C.byref(info)),
             "reverb_rows_plan")
    return _plan_dict(info)


def reverb_rows(pcm, n_samples, rir_bank, rir_taps, rir_delay, rir_index, out=None):
    """pcm float32 [B, n_max] (device), n_samples and rir_index python ints per row; rir_bank float32 [R, taps_max] (device) with
    rir_taps / rir_delay python ints per impulse response -> out [B, n_max]: row b convolved with impulse response rir_index[b],
    shifted by its delay and cut to the row's length, in ONE launch (amdspeech.h: amdspeech_reverb_rows).  A row with index -1 is
    copied bit for bit.  Every word of out is written; input words at or past a row's length are not read."""
    B, n_max = _chk_rows("reverb_rows", pcm, out)
    _chk_f32(rir_bank)
    if rir_bank.dim() != 2 or rir_bank.device != pcm.device:
        raise ValueError("reverb_rows: rir_bank is %s on %s, expected [R, taps_max] beside pcm" % (tuple(rir_bank.shape), rir_bank.device))
    lib = _l.load()
    R, taps_max = rir_bank.shape
    if out is None:
        out = torch.empty_like(pcm)
    ws = _cached_ws(_augment_ws, ("reverb", B, pcm.device), lambda: lib.amdspeech_reverb_rows_workspace_bytes(B))
    _l.check(lib.amdspeech_reverb_rows(_stream(), _p(pcm), _c_ints(n_samples, B, "reverb_rows"), B, n_max, _p(rir_bank),
                                       _c_ints(rir_taps, R, "reverb_rows"), _c_ints(rir_delay, R, "reverb_rows"), R, taps_max,
                                       _c_ints(rir_index, B, "reverb_rows"), _p(out), _p(ws)), "reverb_rows")
    return out          # stream-ordered; the row values were kernel arguments, the cached workspace outlives the kernels


def row_sumsq(pcm, n_samples, out=None):
    """pcm float32 [B, n_max] (device), n_samples python ints -> float64 [B] (device): the sum of squares of each row's first n
    samples, in a fixed order (amdspeech.h: amdspeech_row_sumsq): the same bits every call."""
    B, n_max = _chk_rows("row_sumsq", pcm)
    lib = _l.load()
    if out is None:
        out = torch.empty(B, device=pcm.device, dtype=torch.float64)
    else:
        _chk_f64_vec("row_sumsq: out", out, B, pcm.device)
    ws = _cached_ws(_augment_ws, ("sumsq", B, pcm.device), lambda: lib.amdspeech_row_sumsq_workspace_bytes(B))
    _l.check(lib.amdspeech_row_sumsq(_stream(), _p(pcm), _c_ints(n_samples, B, "row_sumsq"), B, n_max, _p(out), _p(ws)), "row_sumsq")
    return out


def noise_mix_rows_plan(n_samples, n_max, noise_len, m_max, noise_index, noise_offset, snr_decidb):
    """The launch geometry of `noise_mix_rows` (amdspeech.h: amdspeech_noise_mix_rows_plan), as a dict of ints.  Read-only, no device."""
    B, M = len(n_samples), len(noise_len)
    info = _l.NoiseMixRowsPlanInfo()
    what = "noise_mix_rows_plan"
    _l.check(_l.load().amdspeech_noise_mix_rows_plan(_c_ints(n_samples, B, what), B, int(n_max), _c_ints(noise_len, M, what), M, int(m_max),
                                                     _c_ints(noise_index, B, what), _c_ints(noise_offset, B, what),
                                                     _c_ints(snr_decidb, B, what), C.byref(info)), what)
    return _plan_dict(info)


def noise_mix_rows(pcm, n_samples, row_sumsq, noise_bank, noise_len, noise_sumsq, noise_index, noise_offset, snr_decidb, out=None):
    """pcm float32 [B, n_max] (device) with row_sumsq float64 [B] (device, ops.row_sumsq of pcm); noise_bank float32 [M, m_max]
    (device) with noise_len python ints and noise_sumsq float64 [M] (device); noise_index / noise_offset / snr_decidb python ints per
    row -> out: clip noise_index[b], from noise_offset[b] on and wrapping around, added to row b at snr_decidb[b] / 10 dB in ONE launch
    (amdspeech.h: amdspeech_noise_mix_rows).  out None: a new tensor; out = pcm: in place.  A row with index -1, no samples or no
    energy (its own or the clip's) keeps its bits."""
    B, n_max = _chk_rows("noise_mix_rows", pcm, out)
    _chk_f32(noise_bank)
    if noise_bank.dim() != 2 or noise_bank.device != pcm.device:
        raise ValueError("noise_mix_rows: noise_bank is %s on %s, expected [M, m_max] beside pcm" % (tuple(noise_bank.shape), noise_bank.device))
    M, m_max = noise_bank.shape
    _chk_f64_vec("noise_mix_rows: row_sumsq", row_sumsq, B, pcm.device)
    _chk_f64_vec("noise_mix_rows: noise_sumsq", noise_sumsq, M, pcm.device)
    lib = _l.load()
    if out is None:
        out = torch.empty_like(pcm)
    what = "noise_mix_rows"
    ws = _cached_ws(_augment_ws, ("mix", B, pcm.device), lambda: lib.amdspeech_noise_mix_rows_workspace_bytes(B))
    _l.check(lib.amdspeech_noise_mix_rows(_stream(), _p(pcm), _c_ints(n_samples, B, what), B, n_max, _p(noise_bank), _c_ints(noise_len, M, what),
                                          _p(noise_sumsq), M, m_max, _p(row_sumsq), _c_ints(noise_index, B, what),
                                          _c_ints(noise_offset, B, what), _c_ints(snr_decidb, B, what), _p(out), _p(ws)), what)
    return out


def augment_draw(seed, index, reverb_permille, n_rirs, noise_permille, noise_len, snr_decidb):
    """(rir_index, noise_index, noise_offset, snr_decidb) of utterance `index` under `seed`: SpecAugment's integer hash on the host
    (amdspeech.h: amdspeech_augment_draw).  n_rirs impulse responses, clips of noise_len samples, snr_decidb = (lo, hi) inclusive;
    an index of -1: that part is not applied."""
    M = len(noise_len)
    out = (C.c_int * 4)()
    _l.check(_l.load().amdspeech_augment_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(index) & 0xFFFFFFFFFFFFFFFF, int(reverb_permille),
                                              int(n_rirs), int(noise_permille), M, _c_ints(noise_len, M, "augment_draw"),
                                              int(snr_decidb[0]), int(snr_decidb[1]), out), "augment_draw")
    return tuple(out)


def frontend_plan(mode, sample_rate, n_mfcc, B, n_max, t_max):
    """The kernels `frontend` takes for a call (amdspeech.h: amdspeech_frontend_plan), as a dict of ints.  mode "mfcc" / "fbank".
    Read-only: nothing is launched, no device is needed.  A call the front end refuses raises here too."""
    info = _l.FrontendPlanInfo()
    imode = {"mfcc": MODE_MFCC, "fbank": MODE_FBANK}.get(mode, mode)
    _l.check(_l.load().amdspeech_frontend_plan(int(imode), int(sample_rate), int(n_mfcc), int(B), int(n_max), int(t_max), C.byref(info)),
             "frontend_plan")
    return _plan_dict(info)


def frontend(pcm, n_samples, sample_rate, mode, t_max, n_mfcc=20):
    """pcm float32 [B, n_max] (device), n_samples: python ints.  Returns
    (feat [t_max, B, D] device, n_frames list of UNtruncated frame counts)."""
    _chk_f32(pcm)
    lib = _l.load()
    B, n_max = pcm.shape
    imode = MODE_MFCC if mode == "mfcc" else MODE_FBANK
    D = n_mfcc if imode == MODE_MFCC else 120

    def nbytes():
        n = lib.amdspeech_frontend_workspace_bytes(imode, B, n_max, sample_rate)
        if n == 0:
            raise _l.AmdSpeechError("frontend workspace: bad arguments")
        return n

    ws = _cached_ws(_frontend_ws, (imode, B, n_max, sample_rate, pcm.device), nbytes)
    feat = torch.empty(t_max, B, D, device=pcm.device, dtype=torch.float32)
    ns = _c_ints(n_samples, B, "frontend")
    nf = (C.c_int * B)()
    if imode == MODE_MFCC:
        rc = lib.amdspeech_frontend_mfcc(_stream(), _p(pcm), ns, B, n_max, sample_rate, n_mfcc, t_max, _p(feat),
                                         nf, _p(ws))
    else:
        rc = lib.amdspeech_frontend_fbank(_stream(), _p(pcm), ns, B, n_max, sample_rate, t_max, _p(feat), nf,
                                          _p(ws))
    _l.check(rc, "frontend_" + mode)
    return feat, list(nf)          # stream-ordered; the cached workspace outlives the kernels


# ------------------------------------------------------------ low frame rate input
def frame_stack_plan(B, D, t_in, stack, skip):
    """The launch geometry of `frame_stack` for a shape (amdspeech.h: amdspeech_frame_stack_plan), as a dict of ints.  Read-only:
    nothing is launched, no device is needed.  A shape the call refuses raises here too."""
    info = _l.FrameStackPlanInfo()
    _l.check(_l.load().amdspeech_frame_stack_plan(int(B), int(D), int(t_in), int(stack), int(skip), C.byref(info)), "frame_stack_plan")
    return _plan_dict(info)


def frame_stack(feat, n_frames, stack, skip, out=None):
    """feat float32 [t_in, B, D] (device, the front end's output), n_frames: its UNtruncated frame counts (python ints).  Returns
    (out [ceil(t_in / skip), B, stack * D] device, n_out list of ceil(n / skip)): `stack` consecutive frames concatenated, every
    `skip`-th kept, zero from a row's own length on (amdspeech.h: amdspeech_frame_stack)."""
    _chk_f32(out)
    t_in, B, D = _chk_f32_3d("frame_stack", feat, "[t_in, B, D]")
    lib = _l.load()
    nf = _c_ints(n_frames, B, "frame_stack")
    plan = frame_stack_plan(B, D, t_in, stack, skip)
    if out is None:
        out = torch.empty(plan["t_out"], B, plan["d_out"], device=feat.device, dtype=torch.float32)
    elif tuple(out.shape) != (plan["t_out"], B, plan["d_out"]):
        raise ValueError("frame_stack: out is %s, expected %s" % (tuple(out.shape), (plan["t_out"], B, plan["d_out"])))
    no = (C.c_int * B)()
    _l.check(lib.amdspeech_frame_stack(_stream(), _p(feat), nf, B, D, t_in, int(stack), int(skip), _p(out), no), "frame_stack")
    return out, list(no)          # stream-ordered; the lengths were kernel arguments (or the call has waited)


# ------------------------------------------------------------ SpecAugment
SPEC_AUGMENT_KEYS = ("period", "freq_masks", "freq_width", "time_masks", "time_width", "time_permille")


def _spec_augment_desc(policy, seed):
    """policy: a mapping with SPEC_AUGMENT_KEYS (amdspeech.h: amdspeech_spec_augment_desc); seed: 64 bits."""
    missing = [k for k in SPEC_AUGMENT_KEYS if k not in policy]
    if missing:
        raise ValueError("spec_augment: the policy lacks %s" % ", ".join(missing))
    return _l.SpecAugmentDesc(*[int(policy[k]) for k in SPEC_AUGMENT_KEYS], int(seed) & 0xFFFFFFFFFFFFFFFF)


def spec_augment_plan(T, B, W, policy, seed=0):
    """The launch geometry of `spec_augment` for a shape and a policy (amdspeech.h: amdspeech_spec_augment_plan), as a dict of ints;
    workgroups == 0: nothing would be launched.  Read-only: no device is needed.  What the call refuses raises here too."""
    info = _l.SpecAugmentPlanInfo()
    desc = _spec_augment_desc(policy, seed)
    _l.check(_l.load().amdspeech_spec_augment_plan(int(T), int(B), int(W), C.byref(desc), C.byref(info)), "spec_augment_plan")
    return _plan_dict(info)


def spec_augment_spans(policy, seed, row, n):
    """The masks the library draws for row `row` with n = min(length, T) frames under (policy, seed), as (start, width) pairs: the
    policy's freq_masks frequency spans (in bins of the period) first, then its time_masks time spans (in frames).  Host arithmetic."""
    desc = _spec_augment_desc(policy, seed)
    count = max(int(policy["freq_masks"]), 0) + max(int(policy["time_masks"]), 0)
    out = (C.c_int * (2 * max(count, 1)))()
    _l.check(_l.load().amdspeech_spec_augment_spans(C.byref(desc), int(row), int(n), out), "spec_augment_spans")
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(count)]


def spec_augment(x, lengths, policy, seed):
    """x float32 [T, B, W] (device, contiguous), lengths int32 [B] ON THE DEVICE.  Masks x IN PLACE and returns it: frequency and
    time spans of every row's first min(length, T) frames become +0.0, every other word keeps its bit pattern (amdspeech.h:
    amdspeech_spec_augment).  Stream-ordered, no copy, no synchronisation; a policy that can mask nothing launches nothing."""
    T, B, W = _chk_f32_3d("spec_augment", x, "[T, B, W]")
    if not (torch.is_tensor(lengths) and lengths.is_cuda and lengths.device == x.device and lengths.dtype == torch.int32
            and tuple(lengths.shape) == (B,) and lengths.is_contiguous()):
        raise ValueError("spec_augment: lengths must be an int32 device tensor [%d] beside x" % B)
    desc = _spec_augment_desc(policy, seed)
    lib = _l.load()
    info = _l.SpecAugmentPlanInfo()
    _l.check(lib.amdspeech_spec_augment_plan(T, B, W, C.byref(desc), C.byref(info)), "spec_augment")
    if info.workgroups == 0:
        return x
    _l.check(lib.amdspeech_spec_augment(_stream(), _p(x), _p(lengths), T, B, W, C.byref(desc)), "spec_augment")
    return x


# ------------------------------------------------------------ feature normalisation
FEATURE_NORM_VAR_FLOOR = 1e-10


def _feature_norm_mode(mode):
    if mode in _l.FEATURE_NORM_MODES:
        return _l.FEATURE_NORM_MODES.index(mode)
    raise ValueError("feature_norm: mode %r is none of %s" % (mode, ", ".join(_l.FEATURE_NORM_MODES)))


def feature_norm_plan(B, D, t_in, mode="utterance"):
    """The launch geometry of `feature_norm` / `feature_moments` for a shape (amdspeech.h: amdspeech_feature_norm_plan), as a dict of
    ints.  Read-only: nothing is launched, no device is needed.  A shape the calls refuse raises here too."""
    info = _l.FeatureNormPlanInfo()
    _l.check(_l.load().amdspeech_feature_norm_plan(int(B), int(D), int(t_in), _feature_norm_mode(mode), C.byref(info)), "feature_norm_plan")
    return _plan_dict(info)


def _feature_norm_args(what, feat, n_frames):
    t_in, B, D = _chk_f32_3d(what, feat, "[t_in, B, D]")
    nf = _c_ints(n_frames, B, what)
    plan = feature_norm_plan(B, D, t_in, "utterance")
    ws = torch.empty(max(plan["workspace_bytes"], 8), device=feat.device, dtype=torch.uint8)
    return t_in, B, D, nf, ws


def feature_moments(feat, n_frames):
    """feat float32 [t_in, B, D] (device, the front end's output), n_frames: its UNtruncated frame counts (python ints).  Returns a
    float64 device tensor [B, 2, D]: per row the mean and M2 = sum (x - mean)^2 over its first min(n, t_in) frames, zeros for an
    empty row (amdspeech.h: amdspeech_feature_moments).  feat is not written."""
    t_in, B, D, nf, ws = _feature_norm_args("feature_moments", feat, n_frames)
    out = torch.empty(B, 2, D, device=feat.device, dtype=torch.float64)
    _l.check(_l.load().amdspeech_feature_moments(_stream(), _p(feat), nf, B, D, t_in, _p(ws), _p(out)), "feature_moments")
    return out          # stream-ordered; the lengths were kernel arguments (or the call has waited)


def feature_norm(feat, n_frames, mode, norm_vars=True, var_floor=FEATURE_NORM_VAR_FLOOR, table=None):
    """Normalises feat float32 [t_in, B, D] (device, the front end's output) IN PLACE over each row's first min(n, t_in) frames and
    returns it (amdspeech.h: amdspeech_feature_norm).  mode "utterance": mean and population variance of the row itself; "global":
    table, a float64 device tensor [2, D] of means and scales (FeatureStats.table) -- norm_vars and var_floor are then part of the
    table; "none": nothing is launched.  Frames at or past a row's length are neither read nor written."""
    imode = _feature_norm_mode(mode)
    if imode == 0:
        return feat
    t_in, B, D, nf, ws = _feature_norm_args("feature_norm", feat, n_frames)
    if imode == 2:
        if not (torch.is_tensor(table) and table.is_cuda and table.device == feat.device and table.dtype == torch.float64
                and tuple(table.shape) == (2, D) and table.is_contiguous()):
            raise ValueError("feature_norm: global mode needs a float64 device table [2, %d] beside feat" % D)
    elif table is not None:
        raise ValueError("feature_norm: a table belongs to global mode only")
    desc = _l.FeatureNormDesc(imode, int(bool(norm_vars)), float(var_floor))
    _l.check(_l.load().amdspeech_feature_norm(_stream(), _p(feat), nf, B, D, t_in, C.byref(desc), _p(table), _p(ws)), "feature_norm")
    return feat


# ------------------------------------------------------------ lookahead convolution
LOOKAHEAD_MAX_CONTEXT = 32


def lookahead_plan(T, B, H, context):
    """The launch geometry of `lookahead_fwd` / `lookahead_bwd` for a shape (amdspeech.h: amdspeech_lookahead_plan), as a dict of ints
    with "workspace_bytes" (amdspeech_lookahead_bwd_workspace_bytes) beside the struct's fields.  Read-only: nothing is launched, no
    device is needed.  A shape the calls refuse raises here too."""
    info = _l.LookaheadPlanInfo()
    lib = _l.load()
    _l.check(lib.amdspeech_lookahead_plan(int(T), int(B), int(H), int(context), C.byref(info)), "lookahead_plan")
    out = _plan_dict(info)
    out["workspace_bytes"] = int(lib.amdspeech_lookahead_bwd_workspace_bytes(int(T), int(B), int(H), int(context)))
    return out


class LookaheadWorkspace(object):
    """The partial weight-gradient tiles of lookahead_bwd for calls of up to T frames (a shorter run length needs no more).  The call
    writes every word it reads: no fill."""

    def __init__(self, T, B, H, context, device="cuda"):
        self.shape = (T, B, H, context)
        n = lookahead_plan(T, B, H, context)["workspace_bytes"]
        self.buf = torch.empty(max(n, 16), device=device, dtype=torch.uint8)

    def fits(self, T, B, H, context):
        return self.shape[1:] == (B, H, context) and T <= self.shape[0]


def _lookahead_args(what, x, w, lengths, others):
    T, B, H = _chk_f32_3d(what, x, "[T, B, H]")
    _chk_f32(w, *others)
    _chk_i32(lengths)
    if w.dim() != 2 or w.shape[1] != H or w.shape[0] < 2:
        raise ValueError("%s: w %s is not [context + 1, %d]" % (what, tuple(w.shape), H))
    if lengths.numel() != B:
        raise ValueError("%s: %d lengths for %d rows" % (what, lengths.numel(), B))
    for t in others:
        if t is not None and tuple(t.shape) != (T, B, H):
            raise ValueError("%s: a tensor of shape %s beside x %s" % (what, tuple(t.shape), (T, B, H)))
    return T, B, H, w.shape[0] - 1


def lookahead_fwd(x, w, lengths, out=None):
    """y [T,B,H] = the row convolution of x [T,B,H] with w [context+1, H] over each row's own frames, zeros past its length
    (amdspeech.h: amdspeech_lookahead_fwd).  lengths: int32 [B] on the device."""
    T, B, H, context = _lookahead_args("lookahead_fwd", x, w, lengths, (out,))
    if out is None:
        out = torch.empty_like(x)
    _l.check(_l.load().amdspeech_lookahead_fwd(_stream(), _p(x), _p(w), _p(lengths), T, B, H, context, _p(out)), "lookahead_fwd")
    return out


def lookahead_bwd(x, w, dy, lengths, dx=None, dw=None, ws=None):
    """dx [T,B,H] (written in every element) and dw [context+1, H] += the weight gradient (amdspeech.h: amdspeech_lookahead_bwd).
    Returns (dx, dw); a dw made here starts from zeros."""
    T, B, H, context = _lookahead_args("lookahead_bwd", x, w, lengths, (dy, dx))
    if dy is None:
        raise ValueError("lookahead_bwd: dy is required")
    _chk_f32(dw)
    if dx is None:
        dx = torch.empty_like(x)
    if dw is None:
        dw = torch.zeros_like(w)
    if tuple(dw.shape) != tuple(w.shape):
        raise ValueError("lookahead_bwd: dw %s beside w %s" % (tuple(dw.shape), tuple(w.shape)))
    if ws is None or not ws.fits(T, B, H, context):
        ws = LookaheadWorkspace(T, B, H, context, x.device)
    _l.check(_l.load().amdspeech_lookahead_bwd(_stream(), _p(x), _p(w), _p(dy), _p(lengths), T, B, H, context, _p(dx), _p(dw), _p(ws.buf)),
             "lookahead_bwd")
    return dx, dw


# ------------------------------------------------------------ time-frequency convolution (front)
CONV2D_CHANNELS = (16, 32, 48, 64)
CONV2D_MAX_KT, CONV2D_MAX_KF, CONV2D_MAX_STRIDE, CONV2D_MAX_WIDTH = 11, 41, 4, 4096


def conv2d_out_shape(T, F, C, st, sf):
    """(T', F' * C): model frames and input-Linear width behind the convolution."""
    return -(-int(T) // int(st)), -(-int(F) // int(sf)) * int(C)


def conv2d_check(C, kt, kf, st, sf, F=None):
    """The ranges of the layer's sizes (amdspeech.h), as a ValueError that says which one is wrong; with F also the output width."""
    if C not in CONV2D_CHANNELS:
        raise ValueError("conv_channels must be 0 (off) or one of %s, not %r" % (", ".join(map(str, CONV2D_CHANNELS)), C))
    if not (1 <= kt <= CONV2D_MAX_KT and 1 <= kf <= CONV2D_MAX_KF):
        raise ValueError("conv_kernel %d, %d: time taps 1 .. %d, frequency taps 1 .. %d" % (kt, kf, CONV2D_MAX_KT, CONV2D_MAX_KF))
    if kt % 2 == 0 or kf % 2 == 0:
        raise ValueError("conv_kernel %d, %d: both sizes must be odd (the padding is (k - 1) / 2 on each side)" % (kt, kf))
    if not (1 <= st <= CONV2D_MAX_STRIDE and 1 <= sf <= CONV2D_MAX_STRIDE):
        raise ValueError("conv_stride %d, %d: each 1 .. %d" % (st, sf, CONV2D_MAX_STRIDE))
    if F is not None and conv2d_out_shape(1, F, C, st, sf)[1] > CONV2D_MAX_WIDTH:
        raise ValueError("conv: %d output bins x %d channels = %d inputs of the input layer, more than %d"
                         % (-(-F // sf), C, conv2d_out_shape(1, F, C, st, sf)[1], CONV2D_MAX_WIDTH))


def conv2d_plan(T, B, G, F, C, kt, kf, st, sf):
    """The launch geometry of `conv2d_fwd` / `conv2d_bwd` for a shape (amdspeech.h: amdspeech_conv2d_plan), as a dict of ints with
    "workspace_bytes" (amdspeech_conv2d_bwd_workspace_bytes) beside the struct's fields.  Read-only: nothing is launched, no device
    is needed.  A shape the calls refuse raises here too."""
    info = _l.Conv2dPlanInfo()
    lib = _l.load()
    dims = [int(v) for v in (T, B, G, F, C, kt, kf, st, sf)]
    _l.check(lib.amdspeech_conv2d_plan(*dims, _l.C.byref(info)), "conv2d_plan")      # (the parameter C hides this module's ctypes)
    out = _plan_dict(info)
    out["workspace_bytes"] = int(lib.amdspeech_conv2d_bwd_workspace_bytes(*dims))
    return out


class Conv2dWorkspace(object):
    """The partial weight-gradient tiles of conv2d_bwd for calls of up to T source frames (a shorter run needs no more).  The call
    writes every word it reads: no fill."""

    def __init__(self, T, B, G, F, C, kt, kf, st, sf, device="cuda"):
        self.shape = (T, B, G, F, C, kt, kf, st, sf)
        n = conv2d_plan(*self.shape)["workspace_bytes"]
        self.buf = torch.empty(max(n, 16), device=device, dtype=torch.uint8)

    def fits(self, T, *rest):
        return self.shape[1:] == tuple(rest) and T <= self.shape[0]


def _conv2d_args(what, x, w, G, kernel, stride):
    T, B, D = _chk_f32_3d(what, x, "[T, B, G * F]")
    _chk_f32(w)
    (kt, kf), (st, sf) = kernel, stride
    if w.dim() != 2 or D % G != 0 or w.shape[0] != G * kt * kf:
        raise ValueError("%s: w %s is not [%d * %d * %d, C] for x %s" % (what, tuple(w.shape), G, kt, kf, tuple(x.shape)))
    return T, B, D // G, w.shape[1], kt, kf, st, sf


def conv2d_fwd(x, w, bias, lengths, G, kernel, stride, out=None, lengths_out=None):
    """(y [T', B, F' * C], lengths_out int32 [B]) = the strided "same" convolution of x [T, B, G * F] with w [G * kt * kf, C], + bias,
    clipped to 0 .. 20, zeros past each row's ceil(length / st) (amdspeech.h: amdspeech_conv2d_fwd).  lengths: int32 [B] on the device."""
    T, B, F, C, kt, kf, st, sf = _conv2d_args("conv2d_fwd", x, w, G, kernel, stride)
    _chk_f32(bias, out)
    _chk_i32(lengths)
    To, W = conv2d_out_shape(T, F, C, st, sf)
    if out is None:
        out = torch.empty(To, B, W, device=x.device, dtype=torch.float32)
    if lengths_out is None:
        lengths_out = torch.empty(B, device=x.device, dtype=torch.int32)
    _chk_i32(lengths_out)
    if tuple(out.shape) != (To, B, W) or lengths.numel() != B or lengths_out.numel() != B or tuple(bias.shape) != (C,):
        raise ValueError("conv2d_fwd: out %s / lengths %d / bias %s beside x %s, w %s" % (tuple(out.shape), lengths.numel(), tuple(bias.shape),
                                                                                      tuple(x.shape), tuple(w.shape)))
    _l.check(_l.load().amdspeech_conv2d_fwd(_stream(), _p(x), _p(w), _p(bias), _p(lengths), T, B, G, F, C, kt, kf, st, sf, _p(out),
                                            _p(lengths_out)), "conv2d_fwd")
    return out, lengths_out


def conv2d_bwd(x, y, dy, lengths, G, kernel, stride, dw, db, ws=None):
    """dw [G * kt * kf, C] += and db [C] += the layer's gradients from its input x, its output y (the activation's mask is read from
    it) and dy (amdspeech.h: amdspeech_conv2d_bwd).  lengths are the SOURCE lengths.  Returns (dw, db)."""
    T, B, F, C, kt, kf, st, sf = _conv2d_args("conv2d_bwd", x, dw, G, kernel, stride)
    _chk_f32(y, dy, db)
    _chk_i32(lengths)
    To, W = conv2d_out_shape(T, F, C, st, sf)
    if tuple(y.shape) != (To, B, W) or tuple(dy.shape) != (To, B, W) or lengths.numel() != B or tuple(db.shape) != (C,):
        raise ValueError("conv2d_bwd: y %s / dy %s / db %s beside x %s, dw %s" % (tuple(y.shape), tuple(dy.shape), tuple(db.shape),
                                                                                 tuple(x.shape), tuple(dw.shape)))
    if ws is None or not ws.fits(T, B, G, F, C, kt, kf, st, sf):
        ws = Conv2dWorkspace(T, B, G, F, C, kt, kf, st, sf, x.device)
    _l.check(_l.load().amdspeech_conv2d_bwd(_stream(), _p(x), _p(y), _p(dy), _p(lengths), T, B, G, F, C, kt, kf, st, sf, _p(dw), _p(db),
                                            _p(ws.buf)), "conv2d_bwd")
    return dw, db


# ------------------------------------------------------------ voice activity / long recordings
_vad_ws = {}


def vad_num_frames(n_samples, hop):
    """ceil(n_samples / hop): the frames of a row (amdspeech.h: amdspeech_vad_num_frames).  Host arithmetic."""
    got = _l.load().amdspeech_vad_num_frames(int(n_samples), int(hop))
    if got < 0:
        _l.check(got, "vad_num_frames")
    return got


def vad_plan(B, n_max, hop):
    """The launch geometry of `vad_energy` / `vad_flags` for a shape (amdspeech.h: amdspeech_vad_plan), as a dict of ints.
    Read-only: nothing is launched, no device is needed.  A shape the calls refuse raises here too."""
    info = _l.VadPlanInfo()
    _l.check(_l.load().amdspeech_vad_plan(int(B), int(n_max), int(hop), C.byref(info)), "vad_plan")
    return _plan_dict(info)


def _chk_rows_2d(what, t, dtype, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous %s device matrix" % (what, name, dtype))
    return t.shape


def vad_energy(pcm, n_samples, hop, out=None):
    """pcm float32 [B, n_max] (device), n_samples python ints, hop samples per block -> energy_db float32 [B, f_max] (device), f_max =
    ceil(n_max / hop): the decibels of the mean square of two blocks per frame, -120 past a row's frames (amdspeech.h:
    amdspeech_vad_energy).  Words of pcm at or past a row's length are not read.  out: an [B, >= f_max] tensor to fill."""
    B, n_max = _chk_rows_2d("vad_energy", pcm, torch.float32, "pcm")
    lib = _l.load()
    ns = _c_ints(n_samples, B, "vad_energy")
    if out is None:
        out = torch.empty(B, vad_plan(B, n_max, hop)["f_max"], device=pcm.device, dtype=torch.float32)
    elif _chk_rows_2d("vad_energy", out, torch.float32, "out")[0] != B or out.device != pcm.device:
        raise ValueError("vad_energy: out is %s on %s, expected [%d, f_max] beside pcm" % (tuple(out.shape), out.device, B))
    _l.check(lib.amdspeech_vad_energy(_stream(), _p(pcm), ns, B, n_max, int(hop), _p(out), out.shape[1], None), "vad_energy")
    return out          # stream-ordered; the lengths were kernel arguments (or the call has waited)


def vad_flags(energy_db, n_frames, percentile=10, margin_db=10.0, range_db=50.0, min_db=-70.0, min_run=5, hangover=20, speech=None,
              stats=None):
    """energy_db float32 [B, f_max] (device, vad_energy's output), n_frames python ints -> (speech uint8 [B, f_max], stats float32
    [B, 3] = floor, peak, threshold), both on the device: frames above the adaptive threshold and above min_db, runs shorter than
    min_run frames cleared, the rest widened by hangover frames (amdspeech.h: amdspeech_vad_flags).  speech / stats: tensors to fill."""
    B, f_max = _chk_rows_2d("vad_flags", energy_db, torch.float32, "energy_db")
    lib = _l.load()
    nf = _c_ints(n_frames, B, "vad_flags")
    if speech is None:
        speech = torch.empty(B, f_max, device=energy_db.device, dtype=torch.uint8)
    elif tuple(_chk_rows_2d("vad_flags", speech, torch.uint8, "speech")) != (B, f_max) or speech.device != energy_db.device:
        raise ValueError("vad_flags: speech is %s, expected %s beside energy_db" % (tuple(speech.shape), (B, f_max)))
    if stats is None:
        stats = torch.empty(B, 3, device=energy_db.device, dtype=torch.float32)
    elif tuple(_chk_rows_2d("vad_flags", stats, torch.float32, "stats")) != (B, 3) or stats.device != energy_db.device:
        raise ValueError("vad_flags: stats is %s, expected %s beside energy_db" % (tuple(stats.shape), (B, 3)))
    ws = _cached_ws(_vad_ws, (B, f_max, energy_db.device), lambda: max(lib.amdspeech_vad_workspace_bytes(B, f_max, 1), 4))
    _l.check(lib.amdspeech_vad_flags(_stream(), _p(energy_db), nf, B, f_max, int(percentile), float(margin_db), float(range_db),
                                     float(min_db), int(min_run), int(hangover), _p(speech), _p(stats), _p(ws)), "vad_flags")
    return speech, stats          # stream-ordered; the cached workspace outlives the kernels


def gather_spans(pcm, n_samples, row, start, count, w_out, out=None):
    """pcm float32 [B, n_max] (device), n_samples python ints; row / start / count: python ints per span -> out float32 [S, w_out]
    (device): out[s, i] = pcm[row[s], start[s] + i] for i < min(count[s], n_samples[row[s]] - start[s], w_out), zero from there
    on, in ONE launch (amdspeech.h: amdspeech_gather_spans).  No span reads past its row's length.  out: an [S, w_out] tensor to fill."""
    B, n_max = _chk_rows_2d("gather_spans", pcm, torch.float32, "pcm")
    S = len(row)
    ns = _c_ints(n_samples, B, "gather_spans")
    rows, starts, counts = (_c_ints(v, S, "gather_spans") for v in (row, start, count))
    if out is None:
        out = torch.empty(S, max(int(w_out), 1), device=pcm.device, dtype=torch.float32)
    elif tuple(_chk_rows_2d("gather_spans", out, torch.float32, "out")) != (S, int(w_out)) or out.device != pcm.device:
        raise ValueError("gather_spans: out is %s, expected %s beside pcm" % (tuple(out.shape), (S, int(w_out))))
    _l.check(_l.load().amdspeech_gather_spans(_stream(), _p(pcm), ns, B, n_max, rows, starts, counts, S, _p(out) if S else None,
                                              int(w_out)), "gather_spans")
    return out          # stream-ordered; the spans were kernel arguments (or the call has waited)


# ---------------------------------------------------------------- language model
_embed_ws = {}
_xent_ws = {}


def _chk_tokens(what, tok, lengths, T, B):
    """tok: int32 device matrix [B, >= T] with contiguous rows (a column-shifted view of a wider buffer is fine); returns its ld."""
    if not (torch.is_tensor(tok) and tok.is_cuda and tok.dtype == torch.int32 and tok.dim() == 2 and tok.shape[0] == B
            and tok.shape[1] >= T and (tok.shape[1] == 1 or tok.stride(1) == 1) and (B == 1 or tok.stride(0) >= tok.shape[1])):
        raise ValueError("%s: expected an int32 device matrix [%d, >= %d] with contiguous rows" % (what, B, T))
    _chk_i32(lengths)
    if lengths.numel() != B:
        raise ValueError("%s: %d lengths for %d rows" % (what, lengths.numel(), B))
    return tok.stride(0) if B > 1 else max(tok.shape[1], tok.stride(0))


def embed_fwd(tok, lengths, w, bias, out):
    """out [T,B,H] = w[tok[b, t]] + bias inside each row's length, bias elsewhere (amdspeech.h: amdspeech_embed_fwd).  out is
    written in place (the LSTM workspace's Z0 region) and returned."""
    T, B, H = _chk_f32_3d("embed_fwd", out, "[T, B, H]")
    _chk_f32(w, bias)
    ld = _chk_tokens("embed_fwd", tok, lengths, T, B)
    V = w.shape[0]
    if w.dim() != 2 or w.shape[1] != H or (bias is not None and bias.numel() != H):
        raise ValueError("embed_fwd: w %s / bias do not fit H = %d" % (tuple(w.shape), H))
    _l.check(_l.load().amdspeech_embed_fwd(_stream(), _p(tok), ld, _p(lengths), T, B, V, H, _p(w), _p(bias), _p(out)), "embed_fwd")
    return out


def embed_bwd(tok, lengths, dz, dw, dbias):
    """dw [V,H] += the rows of dz [T,B,H] summed per token, dbias [H] (or None) += their sum: no atomics, a fixed order
    (amdspeech.h: amdspeech_embed_bwd)."""
    T, B, H = _chk_f32_3d("embed_bwd", dz, "[T, B, H]")
    _chk_f32(dw, dbias)
    ld = _chk_tokens("embed_bwd", tok, lengths, T, B)
    V = dw.shape[0]
    if dw.dim() != 2 or dw.shape[1] != H or (dbias is not None and dbias.numel() != H):
        raise ValueError("embed_bwd: dw %s / dbias do not fit H = %d" % (tuple(dw.shape), H))
    lib = _l.load()
    ws = _cached_ws(_embed_ws, (T, B, V, H, dz.device), lambda: max(int(lib.amdspeech_embed_bwd_workspace_bytes(T, B, V, H)), 16))
    _l.check(lib.amdspeech_embed_bwd(_stream(), _p(tok), ld, _p(lengths), T, B, V, H, _p(dz), _p(dw), _p(dbias), _p(ws)), "embed_bwd")


def xent_plan(T, B, C_):
    """The row kernel xent_fwd_bwd takes for a shape (amdspeech.h: amdspeech_xent_plan), as a dict of ints with "kernel" as a name
    ("wave", "block").  Read-only: nothing is launched.  A shape the call refuses raises here too."""
    info = _l.XentPlanInfo()
    _l.check(_l.load().amdspeech_xent_plan(int(T), int(B), int(C_), C.byref(info)), "xent_plan")
    out = _plan_dict(info)
    out["kernel"] = _l.XENT_KERNELS[out["kernel"]]
    return out


def xent_fwd_bwd(logits, targets, lengths, scale=1.0, nll=None, loss=None, dlogits=None, want_nll=False, want_grad=True):
    """Softmax cross-entropy of logits [T,B,C] against targets int32 [B, >= T] (amdspeech.h: amdspeech_xent_fwd_bwd).  Returns
    (loss [B], nll [T,B] or None, dlogits [T,B,C] or None); dlogits may be `logits` itself.  want_grad=False is the scoring call."""
    T, B, C_ = _chk_f32_3d("xent_fwd_bwd", logits, "[T, B, C]")
    _chk_f32(nll, loss, dlogits)
    ld = _chk_tokens("xent_fwd_bwd", targets, lengths, T, B)
    dev = logits.device
    if loss is None:
        loss = torch.empty(B, device=dev, dtype=torch.float32)
    if nll is None and want_nll:
        nll = torch.empty(T, B, device=dev, dtype=torch.float32)
    if dlogits is None and want_grad:
        dlogits = torch.empty_like(logits)
    lib = _l.load()
    ws = _cached_ws(_xent_ws, (T, B, C_, dev), lambda: max(int(lib.amdspeech_xent_workspace_bytes(T, B, C_)), 16))
    _l.check(lib.amdspeech_xent_fwd_bwd(_stream(), _p(logits), _p(targets), ld, _p(lengths), T, B, C_, float(scale), _p(nll), _p(loss),
                                        _p(dlogits), _p(ws)), "xent_fwd_bwd")
    return loss, nll, dlogits


def lm_step_plan(N, L, H, V):
    """The instantiation lm_step takes for a shape (amdspeech.h: amdspeech_lm_step_plan), as a dict of ints with "kernel" as a
    name; n_min .. n_max is the range of N on the same instantiation.  Read-only, no device needed; a refused shape raises."""
    info = _l.LmStepPlanInfo()
    _l.check(_l.load().amdspeech_lm_step_plan(int(N), int(L), int(H), int(V), C.byref(info)), "lm_step_plan")
    out = _plan_dict(info)
    out["kernel"] = _l.LM_STEP_KERNELS[out["kernel"]]
    return out


def lm_step(parent, token, dest, pool_h, pool_c, input_w, input_b, kernel_0, kernel_stride, bias_0, bias_stride, output_w, output_b,
            logq=None):
    """One language-model step for N hypotheses (amdspeech.h: amdspeech_lm_step): parent / token / dest int32 device [N], the state
    pool pool_h / pool_c float32 device [n_slots, L, H] (written in place at the dest slots), the parameters as ParamLayout(L, H, V,
    V) views.  Returns logq [N, V], the natural-log next-token distribution of every row.  The slot contract (dest distinct, no dest
    among the parents) is the caller's: language_model.LmStepper checks it on its host copies."""
    _chk_i32(parent, token, dest)
    _chk_f32(pool_h, pool_c, input_w, input_b, kernel_0, bias_0, output_w, output_b, logq)
    N = parent.numel()
    if token.numel() != N or dest.numel() != N:
        raise ValueError("lm_step: parent, token and dest must have one entry per row")
    if pool_h.dim() != 3 or pool_h.shape != pool_c.shape:
        raise ValueError("lm_step: pool_h / pool_c must be [n_slots, L, H], got %s / %s" % (tuple(pool_h.shape), tuple(pool_c.shape)))
    n_slots, L, H = pool_h.shape
    V = output_b.numel()
    if tuple(input_w.shape) != (V, H) or input_b.numel() != H or tuple(output_w.shape) != (H, V) or tuple(kernel_0.shape) != (2 * H, 4 * H) \
            or bias_0.numel() != 4 * H:
        raise ValueError("lm_step: the parameters do not fit L = %d, H = %d, V = %d" % (L, H, V))
    if logq is None:
        logq = torch.empty(N, V, device=pool_h.device, dtype=torch.float32)
    elif logq.numel() < N * V:
        raise ValueError("lm_step: logq holds %d values, %d rows of %d need %d" % (logq.numel(), N, V, N * V))
    _l.check(_l.load().amdspeech_lm_step(_stream(), N, _p(parent), _p(token), _p(dest), _p(pool_h), _p(pool_c), n_slots, L, H, V,
                                         _p(input_w), _p(input_b), _p(kernel_0), int(kernel_stride or 0), _p(bias_0), int(bias_stride or 0),
                                         _p(output_w), _p(output_b), _p(logq)), "lm_step")
    return logq


def ctc_beam_search_fused_slots(B, beam_width):
    """State slots ctc_beam_search_fused hands to its `step`: 2 * beam_width per utterance and the root's (the last one)."""
    n = int(_l.load().amdspeech_ctc_beam_search_fused_slots(int(B), int(beam_width)))
    if n <= 0:
        _l.check(-1, "ctc_beam_search_fused_slots")
    return n


def ctc_beam_search_fused(logits, lengths, step, n_best=0, beam_width=100, merge_repeated=True, lm_weight=1.0, lm_length_bonus=0.0,
                          max_threads=0):
    """Host prefix beam search with a language model INSIDE the beam (amdspeech.h: amdspeech_ctc_beam_search_host_fused).
    step(parent, token, dest) -> logq [n, C]: numpy int32 arrays of the n hypotheses to advance (parent slot or -1, the token, the
    slot that receives the new state) in, the model's natural-log next-token rows out; it is called on this thread, once per frame
    for the whole mini-batch.  The model scores the prefix BEFORE merge_repeated.  n_best == 0: (ids [B,T], out_len [B], log_prob
    [B]); otherwise (ids [B,n_best,T], out_len [B,n_best], log_prob [B,n_best], n_found [B]) -- log_prob is the fused score.
    An exception in `step` ends the search and is raised here."""
    import numpy as np
    host = logits.detach().cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits)
    host = np.ascontiguousarray(host, np.float32)
    T, B, C_ = host.shape
    n_best = int(n_best)
    lens = np.ascontiguousarray(lengths.cpu().numpy() if torch.is_tensor(lengths) else lengths, np.int32)
    shape = (B,) if n_best == 0 else (B, n_best)
    ids = np.empty(shape + (T,), np.int32)
    out_len = np.empty(shape, np.int32)
    logp = np.empty(shape, np.float32)
    n_found = np.empty(B, np.int32)
    raised = []

    def trampoline(_user, n, parent, token, dest, logq):
        try:
            q = step(np.ctypeslib.as_array(parent, (n,)).copy(), np.ctypeslib.as_array(token, (n,)).copy(),
                     np.ctypeslib.as_array(dest, (n,)).copy())
            if isinstance(q, int):                      # a status instead of rows: passed through as the call's status
                return q
            q = np.asarray(q, np.float32)
            if q.shape != (n, C_):
                raise ValueError("ctc_beam_search_fused: step returned %s, expected (%d, %d)" % (q.shape, n, C_))
            np.ctypeslib.as_array(logq, (n, C_))[...] = q
            return 0
        except BaseException as e:                      # noqa: B902  (nothing may unwind through the C frames)
            raised.append(e)
            return _l.ECALLBACK

    cb = _l.LM_STEP_FN(trampoline)
    rc = _l.load().amdspeech_ctc_beam_search_host_fused(
        host.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), T, B, C_, int(beam_width), int(bool(merge_repeated)), n_best,
        float(lm_weight), float(lm_length_bonus), cb, None, ids.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p),
        logp.ctypes.data_as(C.c_void_p), n_found.ctypes.data_as(C.c_void_p), int(max_threads))
    if raised:
        raise raised[0]
    _l.check(rc, "ctc_beam_search_host_fused")
    return (ids, out_len, logp) if n_best == 0 else (ids, out_len, logp, n_found)


# ---------------------------------------------------------------- transducer
_rnnt_ws = {}


def rnnt_plan(T, B, U, J, C_):
    """The instantiations and launch geometry of the transducer calls for a shape (amdspeech.h: amdspeech_rnnt_plan), as a dict of
    ints with "rec_kernel" as a name ("wave", "block1", "block4", "block10") and "workspace_bytes" added.  Read-only, no device
    needed; a refused shape raises."""
    info = _l.RnntPlanInfo()
    lib = _l.load()
    _l.check(lib.amdspeech_rnnt_plan(int(T), int(B), int(U), int(J), int(C_), C.byref(info)), "rnnt_plan")
    out = _plan_dict(info)
    out["rec_kernel"] = _l.RNNT_REC_KERNELS[out["rec_kernel"]]
    out["workspace_bytes"] = int(lib.amdspeech_rnnt_workspace_bytes(int(T), int(B), int(U), int(J), int(C_)))
    return out


def rnnt_workspace(T, B, U, J, C_, device):
    """The (cached) workspace rnnt_loss_fwd_bwd and rnnt_joint_bwd share for a shape."""
    lib = _l.load()
    return _cached_ws(_rnnt_ws, (T, B, U, J, C_, device), lambda: max(int(lib.amdspeech_rnnt_workspace_bytes(T, B, U, J, C_)), 256))


def rnnt_targets(dense_labels, C_):
    """dense_labels int32 [B, U] -> (targets [B, U], n [B], tok [B, U+2], tok_len [B]) (amdspeech.h: amdspeech_rnnt_targets)."""
    _chk_i32(dense_labels)
    if dense_labels.dim() != 2:
        raise ValueError("rnnt_targets: dense_labels must be [B, U]")
    B, U = dense_labels.shape
    dev = dense_labels.device
    targets = torch.empty(B, U, device=dev, dtype=torch.int32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    tok = torch.empty(B, U + 2, device=dev, dtype=torch.int32)
    tok_len = torch.empty(B, device=dev, dtype=torch.int32)
    _l.check(_l.load().amdspeech_rnnt_targets(_stream(), _p(dense_labels), B, U, int(C_), _p(targets), _p(n), _p(tok), _p(tok_len)),
             "rnnt_targets")
    return targets, n, tok, tok_len


def _rnnt_shapes(what, f, g, w_out):
    _chk_f32(f, g, w_out)
    if f.dim() != 3 or g.dim() != 3 or w_out.dim() != 2 or g.shape[1:] != f.shape[1:] or w_out.shape[0] != f.shape[2]:
        raise ValueError("%s: f [T, B, J], g [U+1, B, J] and w_out [J, C] do not fit: %s %s %s"
                         % (what, tuple(f.shape), tuple(g.shape), tuple(w_out.shape)))
    T, B, J = f.shape
    return T, B, g.shape[0] - 1, J, w_out.shape[1]


def rnnt_joint_fwd(f, g, w_out, b_out, lengths, n, logits=None):
    """logits [B, T, U+1, C] = tanh(f[t, b] + g[u, b]) . w_out + b_out on every live node (amdspeech.h: amdspeech_rnnt_joint_fwd);
    dead nodes are not written."""
    T, B, U, J, C_ = _rnnt_shapes("rnnt_joint_fwd", f, g, w_out)
    _chk_f32(b_out, logits)
    _chk_i32(lengths, n)
    if b_out.numel() != C_ or lengths.numel() != B or n.numel() != B:
        raise ValueError("rnnt_joint_fwd: b_out, lengths or n do not fit B = %d, C = %d" % (B, C_))
    if logits is None:
        logits = torch.empty(B, T, U + 1, C_, device=f.device, dtype=torch.float32)
    elif logits.numel() != B * T * (U + 1) * C_:
        raise ValueError("rnnt_joint_fwd: logits holds %d values, the lattice has %d" % (logits.numel(), B * T * (U + 1) * C_))
    _l.check(_l.load().amdspeech_rnnt_joint_fwd(_stream(), _p(f), _p(g), _p(w_out), _p(b_out), _p(lengths), _p(n), T, B, U, J, C_,
                                                _p(logits)), "rnnt_joint_fwd")
    return logits


def rnnt_loss_fwd_bwd(logits, targets, n, lengths, loss=None, dlogits=None, ws=None):
    """The transducer loss [B] and dlogits [B, T, U+1, C] of logits (amdspeech.h: amdspeech_rnnt_loss_fwd_bwd); dlogits may be
    `logits` itself."""
    _chk_f32(logits, loss, dlogits)
    _chk_i32(targets, n, lengths)
    if logits.dim() != 4 or targets.dim() != 2 or targets.shape != (logits.shape[0], logits.shape[2] - 1):
        raise ValueError("rnnt_loss_fwd_bwd: logits [B, T, U+1, C] and targets [B, U] do not fit: %s %s"
                         % (tuple(logits.shape), tuple(targets.shape)))
    B, T, U1, C_ = logits.shape
    if n.numel() != B or lengths.numel() != B:
        raise ValueError("rnnt_loss_fwd_bwd: n and lengths must have one entry per row")
    if loss is None:
        loss = torch.empty(B, device=logits.device, dtype=torch.float32)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    if ws is None:
        ws = rnnt_workspace(T, B, U1 - 1, 16, C_, logits.device)
    _l.check(_l.load().amdspeech_rnnt_loss_fwd_bwd(_stream(), _p(logits), _p(targets), _p(n), _p(lengths), T, B, U1 - 1, C_, _p(loss),
                                                   _p(dlogits), _p(ws)), "rnnt_loss_fwd_bwd")
    return loss, dlogits


def rnnt_joint_bwd(dlogits, f, g, w_out, lengths, n, dw_out, db_out, df=None, dg=None, ws=None):
    """df [T, B, J] and dg [U+1, B, J] (overwritten), dw_out / db_out (accumulated) from dlogits (amdspeech.h:
    amdspeech_rnnt_joint_bwd)."""
    T, B, U, J, C_ = _rnnt_shapes("rnnt_joint_bwd", f, g, w_out)
    _chk_f32(dlogits, dw_out, db_out, df, dg)
    _chk_i32(lengths, n)
    if dlogits.numel() != B * T * (U + 1) * C_ or dw_out.shape != w_out.shape or db_out.numel() != C_:
        raise ValueError("rnnt_joint_bwd: dlogits, dw_out or db_out do not fit the lattice")
    if df is None:
        df = torch.empty_like(f)
    if dg is None:
        dg = torch.empty_like(g)
    if df.shape != f.shape or dg.shape != g.shape:
        raise ValueError("rnnt_joint_bwd: df / dg do not fit f / g")
    if ws is None:
        ws = rnnt_workspace(T, B, U, J, C_, f.device)
    _l.check(_l.load().amdspeech_rnnt_joint_bwd(_stream(), _p(dlogits), _p(f), _p(g), _p(w_out), _p(lengths), _p(n), T, B, U, J, C_,
                                                _p(df), _p(dg), _p(dw_out), _p(db_out), _p(ws)), "rnnt_joint_bwd")
    return df, dg


def lm_step_state(parent, token, dest, pool_h, pool_c, input_w, input_b, kernel_0, kernel_stride, bias_0, bias_stride, V):
    """The layer launches of lm_step without the output layer (amdspeech.h: amdspeech_lm_step_state): the same bits in the pool."""
    _chk_i32(parent, token, dest)
    _chk_f32(pool_h, pool_c, input_w, input_b, kernel_0, bias_0)
    N = parent.numel()
    if token.numel() != N or dest.numel() != N:
        raise ValueError("lm_step_state: parent, token and dest must have one entry per row")
    if pool_h.dim() != 3 or pool_h.shape != pool_c.shape:
        raise ValueError("lm_step_state: pool_h / pool_c must be [n_slots, L, H], got %s / %s" % (tuple(pool_h.shape), tuple(pool_c.shape)))
    n_slots, L, H = pool_h.shape
    if tuple(input_w.shape) != (V, H) or input_b.numel() != H or tuple(kernel_0.shape) != (2 * H, 4 * H) or bias_0.numel() != 4 * H:
        raise ValueError("lm_step_state: the parameters do not fit L = %d, H = %d, V = %d" % (L, H, V))
    _l.check(_l.load().amdspeech_lm_step_state(_stream(), N, _p(parent), _p(token), _p(dest), _p(pool_h), _p(pool_c), n_slots, L, H, int(V),
                                               _p(input_w), _p(input_b), _p(kernel_0), int(kernel_stride or 0), _p(bias_0),
                                               int(bias_stride or 0)), "lm_step_state")


def rnnt_greedy_step(f, lengths, U, pool_h, w_pred, b_pred, w_out, b_out, t_idx, m, slot, ids, parent, token, dest):
    """One iteration of greedy transducer decoding for the B rows of f [T, B, J] (amdspeech.h: amdspeech_rnnt_greedy_step); the
    decoding state t_idx / m / slot [B], ids [B, U] and the (parent, token, dest) rows of the following lm_step_state call are
    updated in place."""
    _chk_f32(f, pool_h, w_pred, b_pred, w_out, b_out)
    _chk_i32(lengths, t_idx, m, slot, ids, parent, token, dest)
    T, B, J = f.shape
    if pool_h.dim() != 3 or pool_h.shape[0] != 2 * B:
        raise ValueError("rnnt_greedy_step: pool_h must be [2 B, L, H], got %s" % (tuple(pool_h.shape),))
    _, L, H = pool_h.shape
    C_ = b_out.numel()
    if tuple(w_pred.shape) != (H, J) or b_pred.numel() != J or tuple(w_out.shape) != (J, C_) or tuple(ids.shape) != (B, U) \
            or any(x.numel() != B for x in (lengths, t_idx, m, slot, parent, token, dest)):
        raise ValueError("rnnt_greedy_step: the arguments do not fit B = %d, U = %d, J = %d, C = %d, H = %d" % (B, U, J, C_, H))
    _l.check(_l.load().amdspeech_rnnt_greedy_step(_stream(), _p(f), _p(lengths), T, B, int(U), J, C_, _p(pool_h), L, H, _p(w_pred),
                                                  _p(b_pred), _p(w_out), _p(b_out), _p(t_idx), _p(m), _p(slot), _p(ids), _p(parent),
                                                  _p(token), _p(dest)), "rnnt_greedy_step")
