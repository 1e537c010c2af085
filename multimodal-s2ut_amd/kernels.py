"""Torch-tensor front of the C-ABI: validation + pointer plumbing, no arithmetic.

Every function enqueues HIP kernels on PyTorch's current stream through libmms2ut_hip.so.
Tensors are fp16 (``torch.float16``) unless stated; shapes are checked before the call.
"""
import atexit
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import GemmArgs, call

EPI_F16, EPI_RELU_DROP, EPI_DROP_RESID, EPI_F32, EPI_GATE, EPI_RELU_DROP_BWD, EPI_F16_ACC, EPI_GELU_DROP, \
    EPI_GELU_DROP_BWD = range(9)
F16 = torch.float16


_DEV = [None]


def _dev():
    if _DEV[0] is None:
        _DEV[0] = torch.cuda.current_device()
    return _DEV[0]


def _s():
    """Raw hipStream_t to enqueue on: the side stream inside a side region, else torch's current
    stream (read through the C binding: torch.cuda.current_stream() costs ~5 us per call)."""
    return _Side.override or torch._C._cuda_getCurrentRawStream(_dev())


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, dtype=F16):
    assert t.is_cuda, "HIP kernels need device tensors"
    assert t.dtype == dtype, f"expected {dtype}, got {t.dtype}"


class Dropout:
    """Counter-based dropout stream: each call site draws a disjoint counter range from one
    per-step seed, so a backward pass regenerates exactly the forward mask."""

    def __init__(self, seed=1):
        self.seed = seed
        self.offset = 0

    def reset(self, seed):
        self.seed = int(seed) & ((1 << 63) - 1)
        self.offset = 0

    def take(self, n):
        off = self.offset
        self.offset += (int(n) + 255) // 256 * 256
        return self.seed, off

# ============================================================================ GEMM


def gemm(A, B, C, M, N, K, *, a_kc=True, b_kc=True, lda, ldb, ldc, batch=1, bdiv=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), epi=EPI_F16, alpha=1.0, bias=None, aux=None, ldaux=0,
         sX=(0, 0), out2=None, ldo2=0, p=0.0, seed=0, offset=0, ld_rng=0, splitk=1, sCsplit=0,
         rowsum=None, ld_rowsum=0, fixup=True):
    """One mms2ut_gemm_f16 launch.  The argument block is packed in one struct call (_lib.GEMM_ARGS,
    the C layout of mms2ut_gemm_args).  Short-M fused-epilogue GEMMs take the split-K fixup
    (fixup=False: the unsplit kernel, for tests)."""
    ws_p = ws_n = 0
    if fixup and splitk == 1 and epi != EPI_F32 and batch == 1 and rowsum is None:
        s = _fixup_splits(M, N, K)
        if s > 1:
            ws = _workspace("splitk_fix", s * M * N, C.device)
            splitk, ws_p, ws_n = s, ws.data_ptr(), ws.numel()
    buf = _GEMM_PACK(
        A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, a_kc, b_kc, lda, ldb, ldc, batch, bdiv,
        sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], splitk, sCsplit, epi, alpha,
        0 if bias is None else bias.data_ptr(), 0 if aux is None else aux.data_ptr(), ldaux, sX[0], sX[1],
        0 if out2 is None else out2.data_ptr(), ldo2, p, seed, offset, ld_rng,
        0 if rowsum is None else rowsum.data_ptr(), ld_rowsum, ws_p, ws_n)
    call("mms2ut_gemm_f16", buf, _s())


_GEMM_PACK = _lib.GEMM_ARGS.pack


def _fixup_splits(M, N, K):
    """Split count for a short-M fused-epilogue GEMM (decoder tokens): its 128x128 grid covers a
    fraction of the 256 CUs, so K is split until ~512 workgroups (2 per CU) run, each split keeping
    >= 4 k-tiles (include/mms2ut.h splitk_ws)."""
    if N % 4 or K < 512:
        return 1
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 128:
        return 1
    return max(1, min(512 // tiles, K // 256, 16))


def gemm_profile_begin(max_launches=100000):
    """Start live GEMM timing (HIP events inside the library, on each launch's stream)."""
    call("mms2ut_profile_begin", int(max_launches))


def gemm_profile_end():
    """-> (summed GEMM kernel ms, launches, launched FLOPs, algorithmic HBM bytes)."""
    import ctypes
    ms, n, fl, by = ctypes.c_float(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    call("mms2ut_profile_end", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
    call("mms2ut_profile_bytes", ctypes.byref(by))
    return ms.value, n.value, fl.value, by.value


def gemm_profile_launches(n):
    """Per-launch (ms, launched FLOPs, class word) of the last gemm_profile window (numpy)."""
    import numpy as np
    ms, fl, cls = np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    if n:
        call("mms2ut_profile_launches", ms.ctypes.data, fl.ctypes.data, cls.ctypes.data, int(n))
    return ms, fl, cls


def gemm_profile_shapes(n):
    """[n, 4] int32 (M, N, K, batch * splitk) of the last gemm_profile window's launches."""
    import numpy as np
    mnk = np.zeros((max(n, 0), 4), np.int32)
    if n:
        call("mms2ut_profile_shapes", mnk.ctypes.data, int(n))
    return mnk


def gemm_profile_stamps(buf):
    """Stamp mode for the open profile window: every GEMM kernel's blocks record {start, end}
    s_memrealtime ticks into `buf` (int64 device tensor, 2 per block) instead of HIP events."""
    assert buf.dtype == torch.int64 and buf.is_cuda and buf.numel() % 2 == 0
    call("mms2ut_profile_stamps", buf.data_ptr(), buf.numel() // 2)


def gemm_profile_durations(buf, n):
    """Per-launch kernel durations (ms, numpy float64) of the last stamp-mode window: max(end) -
    min(start) over each launch's blocks; NaN for launches past the buffer's capacity."""
    import ctypes
    import numpy as np
    fl = np.zeros((max(n, 0), 2), np.int64)
    if n:
        call("mms2ut_profile_blocks", fl.ctypes.data, int(n))
    khz = ctypes.c_int()
    call("mms2ut_wallclock_khz", ctypes.byref(khz))
    st = buf.view(-1, 2).cpu().numpy()
    cap = st.shape[0]
    out = np.full(n, np.nan)
    for i, (b0, b1) in enumerate(fl.tolist()):
        if b1 <= cap and b1 > b0:
            out[i] = (st[b0:b1, 1].max() - st[b0:b1, 0].min()) / khz.value   # ticks / kHz = ms
    return out


def linear(x, W, bias=None, out=None, *, epi=EPI_F16, aux=None, out2=None, p=0.0, drop=None,
           ldc=None, alpha=1.0):
    """out[M,N] = epi(x[M,K] @ W[N,K]^T + bias) — nn.Linear forward (fused epilogue)."""
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K, (W.shape, x.shape)
    if out is None:
        out = torch.empty(M, N, dtype=F16, device=x.device)
    seed = off = 0
    if p > 0.0:
        seed, off = drop
    gemm(x, W, out, M, N, K, lda=x.stride(0), ldb=W.stride(0), ldc=ldc or out.stride(0), epi=epi,
         bias=bias, aux=aux, ldaux=(aux.stride(0) if aux is not None else 0), out2=out2,
         ldo2=(out2.stride(0) if out2 is not None else 0), p=p, seed=seed, offset=off, ld_rng=N,
         alpha=alpha)
    return out


class TransposedWeights:
    """W^T images of the weights the backward's dgrad GEMMs read, in one flat fp16 buffer.

    dx = dy @ W reads W [N, K] N-contiguous (transposed LDS reads); with W^T [K, N] both GEMM
    operands are K-contiguous, the NT layout the forward uses (13-20 % faster on the step's dgrad
    shapes, round-2 A/B, scripts/gemm_ab.py in git history).  refresh() re-transposes every registered matrix in one launch on
    the side stream after each optimizer update (it runs beside the forward); the first dgrad of
    the backward makes the main stream wait for it.  linear_dgrad picks the image up by W's
    address and shape; unregistered weights keep the transposed-read path."""
    active = None

    def __init__(self, flat, mats):
        import numpy as np
        base = flat.data_ptr()
        self.flat = flat
        self.lookup = {}
        rows, off, tiles = [], 0, 0
        for W in mats:
            r, c = W.shape
            assert W.dtype == F16 and W.stride(1) == 1 and W.stride(0) == c and r % 8 == 0 and c % 8 == 0
            src = (W.data_ptr() - base) // 2
            if (src, r, c) in self.lookup:
                continue
            self.lookup[(src, r, c)] = off
            rows.append((src, off, r, c, tiles, 0))
            off = round_up(off + r * c, 8)
            tiles += -(-r // 64) * -(-c // 64)
        dt = np.dtype([("src", "<i8"), ("dst", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("tile0", "<i4"),
                       ("pad", "<i4")])
        desc = np.array(rows, dtype=dt)
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(flat.device)
        self.n, self.tiles = len(rows), tiles
        self.flatT = torch.empty(max(off, 8), dtype=F16, device=flat.device)
        self.event = None
        self.waited = True

    def refresh(self):
        if self.n == 0:
            return
        side = side_stream(self.flat.device)
        stream_wait(side, torch.cuda.current_stream(self.flat.device))
        with torch.cuda.stream(side):
            call("mms2ut_transpose_batch", self.flat.data_ptr(), self.flatT.data_ptr(), self.desc.data_ptr(),
                 self.n, self.tiles, _s())
        if self.event is None:
            self.event = DevEvent()
        self.event.record(side)
        self.waited = False

    def get(self, W, wait=True):
        if self.event is None or W.dim() != 2:
            return None
        off = self.lookup.get(((W.data_ptr() - self.flat.data_ptr()) // 2, W.shape[0], W.shape[1]))
        if off is None or W.stride(1) != 1 or W.stride(0) != W.shape[1]:
            return None
        if wait:
            self.wait_ready()
        return self.flatT[off:off + W.numel()].view(W.shape[1], W.shape[0])

    def wait_ready(self):
        """The current stream waits for this step's refresh (once per refresh)."""
        if not self.waited and self.event is not None:
            self.event.wait(torch.cuda.current_stream(self.flat.device))
            self.waited = True


_STREAM_WS = {}


def stream_workspace(numel, device):
    """fp32 scratch private to the current stream (grow-only; a regrown buffer is released to the
    caching allocator on the stream that allocated and used it, so later reuse is stream-ordered).
    In graph mode (_Side.retain) a regrown buffer is retired instead: an earlier captured graph
    still writes its split-K partials into it on every replay."""
    if numel <= 0:
        return None
    key = _s()
    buf = _STREAM_WS.get(key)
    if buf is None or buf.numel() < numel:
        if buf is not None and _Side.retain:
            _Side.retired.append(buf)
        buf = torch.empty(max(numel, 1 << 20), dtype=torch.float32, device=device)
        _STREAM_WS[key] = buf
    return buf


class LayerCall:
    """One pre-LN transformer layer enqueued by a single library call (include/mms2ut.h
    mms2ut_layer_fwd / mms2ut_layer_bwd: the whole per-layer launch sequence from C++ instead of
    ~25 launches issued one by one from Python).  Parameter, gradient and W^T pointers are bound
    once (the flat buffers never move); each forward sets shapes, lengths, dropout offsets and the
    arena, and snapshots the argument block for its backward."""

    _sizes = {}

    def __init__(self, kind, d, H, F, params, grads, dgrad_weights, eps=1e-5):
        a = _lib.LayerArgs()
        a.kind, a.d, a.H, a.F, a.eps = kind, d, H, F, eps
        for f, t in params.items():
            setattr(a, f, t.data_ptr())
        for f, t in grads.items():
            setattr(a, f, t.data_ptr())
        self.a, self.kind, self.d = a, kind, d
        self.dgrad_weights = dgrad_weights     # {"wt_qkv": W [out, in], ...}
        self.wt_of = None

    def _bind_wt(self):
        wt = TransposedWeights.active
        if wt is self.wt_of:
            return
        for f, W in self.dgrad_weights.items():
            img = wt.get(W, wait=False) if wt is not None else None
            setattr(self.a, f, 0 if img is None else img.data_ptr())
        self.wt_of = wt

    def sizes(self):
        a = self.a
        key = (a.kind, a.B, a.T, a.Tk, a.d, a.H, a.F)
        s = LayerCall._sizes.get(key)
        if s is None:
            offs = (ctypes.c_int64 * _lib.LAYER_NSLOT)()
            nb, mw, sw = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            call("mms2ut_layer_arena", ctypes.byref(a), offs, ctypes.byref(nb))
            call("mms2ut_layer_ws", ctypes.byref(a), ctypes.byref(mw), ctypes.byref(sw))
            s = (nb.value, list(offs), mw.value, sw.value, {})
            LayerCall._sizes[key] = s
        return s

    def fwd(self, x, B, T, self_len, seed, p, offs, Tk=0, cross_len=None, kv=None):
        """p = (p_drop, p_attn, p_act); offs = the six site offsets (mms2ut_layer order).
        Returns (arena uint8, byte offsets, argument snapshot)."""
        a = self.a
        a.B, a.T, a.Tk = B, T, Tk
        a.self_len = self_len.data_ptr()
        a.cross_len = cross_len.data_ptr() if cross_len is not None else 0
        a.kv, a.ld_kv = (kv.data_ptr(), kv.stride(0)) if kv is not None else (0, 0)
        a.p_drop, a.p_attn, a.p_act = p
        a.seed = seed
        a.off_sa_attn, a.off_sa_res, a.off_ca_attn, a.off_ca_res, a.off_act, a.off_ffn_res = offs
        a.x = x.data_ptr()
        self._bind_wt()
        nb, offsets, mw, _, _ = self.sizes()
        arena = torch.empty(nb, dtype=torch.uint8, device=x.device)
        a.saved = arena.data_ptr()
        ws = stream_workspace(mw, x.device)
        call("mms2ut_layer_fwd", ctypes.byref(a), None if ws is None else ws.data_ptr(), mw, _s())
        return arena, offsets, bytes(a)

    @staticmethod
    def view(arena, offsets, slot, shape, dtype=F16):
        n = 1
        for s in shape:
            n *= s
        o = offsets[slot]
        return arena[o:o + n * torch.tensor([], dtype=dtype).element_size()].view(dtype).view(shape)

    def bwd(self, snap, arena, dy, R, dy_drop=None, emit=None, dkv=None, last=False):
        """Backward of the forward whose argument snapshot is ``snap``.  emit = (p, (seed, offset)):
        also return dropout(dx) for the layer below.  last: nothing follows on the critical path
        (the weight gradients may take the whole chip).  Returns (dx, dropout(dx) or dx)."""
        emit_p, (emit_seed, emit_off) = (emit[0], emit[1]) if emit is not None and emit[0] > 0 else (0.0, (0, 0))
        nb, offsets, mw, sw, scr = self.sizes()
        sk = emit_p > 0
        s = scr.get(sk)
        if s is None:
            dxo, sb = (ctypes.c_int64 * 2)(), ctypes.c_int64()
            call("mms2ut_layer_scratch", ctypes.byref(self.a), float(emit_p), dxo, ctypes.byref(sb))
            s = scr[sk] = (sb.value, list(dxo))
        sbytes, dxo = s
        dev = dy.device
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        if TransposedWeights.active is not None:
            TransposedWeights.active.wait_ready()
        main_ws = stream_workspace(mw, dev)
        side = 0
        if _Side.enabled:
            side_stream(dev)
            side = _Side.ptr
            with _SIDE_REGION:
                side_ws = _workspace("layer_side", sw, dev)
        else:
            side_ws = _workspace("layer_side", sw, dev) if sw > 0 else None
        g = _lib.LAYER_GRAD_ARGS.pack(
            dy.data_ptr(), 0 if dy_drop is None else dy_drop.data_ptr(), float(emit_p), int(emit_seed),
            int(emit_off), 0 if dkv is None else dkv.data_ptr(), 0 if dkv is None else dkv.stride(0),
            scratch.data_ptr(), 0 if main_ws is None else main_ws.data_ptr(), mw,
            0 if side_ws is None else side_ws.data_ptr(), sw, 0 if last else SIDE_WGRAD_BLOCKS)
        call("mms2ut_layer_bwd", snap, g, _s(), side)
        if side:
            # the side stream reads the arena (saved activations), the scratch and the incoming
            # gradient (dy / its dropout: the grouped fc2 weight gradient runs after the layer's
            # whole dgrad chain): keep them until side_join; nothing else may reuse them before
            _Side.keep.extend((arena, scratch, dy) if dy_drop is None else (arena, scratch, dy, dy_drop))
            _Side.used = True
        d = self.d
        dx = scratch[dxo[0]:dxo[0] + 2 * R * d].view(F16).view(R, d)
        dxd = scratch[dxo[1]:dxo[1] + 2 * R * d].view(F16).view(R, d) if sk else dx
        return dx, dxd


class ConvCall:
    """The Conv1d subsampler enqueued by one library call each way (include/mms2ut.h
    mms2ut_conv1d_glu_fwd / _bwd: im2col, projection GEMM, GLU per layer from C++, the weight
    gradients on the side stream).  Weight / gradient / W^T pointers are bound once; each forward
    sets the batch shape and the arena and snapshots the argument block for its backward."""

    _sizes = {}

    def __init__(self, ks, couts, weights, biases, gweights, gbiases, dgrad_weights):
        a = _lib.ConvArgs()
        a.nlayers = len(ks)
        for i, k in enumerate(ks):
            a.k[i], a.cout[i] = k, couts[i]
            a.w[i], a.b[i] = weights[i].data_ptr(), biases[i].data_ptr()
            a.g_w[i], a.g_b[i] = gweights[i].data_ptr(), gbiases[i].data_ptr()
        self.a = a
        self.dgrad_weights = dgrad_weights     # {layer: W viewed [cout, C k]} for layers >= 1
        self.wt_of = None

    def _bind_wt(self):
        wt = TransposedWeights.active
        if wt is self.wt_of:
            return
        for i, W in self.dgrad_weights.items():
            img = wt.get(W, wait=False) if wt is not None else None
            self.a.wt[i] = 0 if img is None else img.data_ptr()
        self.wt_of = wt

    def sizes(self, a=None):
        """Arena / scratch / workspace sizes of the call described by `a` (the live argument block
        by default; a backward passes its forward's snapshot, which a later forward of the same
        call may have overwritten in self.a)."""
        a = self.a if a is None else a
        key = (a.B, a.T, a.C, a.nlayers, tuple(a.k), tuple(a.cout))
        s = ConvCall._sizes.get(key)
        if s is None:
            out_off, nb, sb, dxo = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            mw, sw = ctypes.c_int64(), ctypes.c_int64()
            call("mms2ut_conv1d_glu_arena", ctypes.byref(a), ctypes.byref(out_off), ctypes.byref(nb))
            call("mms2ut_conv1d_glu_scratch", ctypes.byref(a), ctypes.byref(dxo), ctypes.byref(sb))
            call("mms2ut_conv1d_glu_ws", ctypes.byref(a), ctypes.byref(mw), ctypes.byref(sw))
            s = (nb.value, out_off.value, sb.value, mw.value, sw.value)
            ConvCall._sizes[key] = s
        return s

    def fwd(self, x, B, T, C):
        """x [B*T, C] fp16 -> (arena, output [B*T_out, cout_last / 2] view, argument snapshot)."""
        a = self.a
        a.B, a.T, a.C = B, T, C
        a.x = x.data_ptr()
        self._bind_wt()
        nb, out_off, _, mw, _ = self.sizes()
        arena = torch.empty(nb, dtype=torch.uint8, device=x.device)
        a.saved = arena.data_ptr()
        ws = stream_workspace(mw, x.device)
        call("mms2ut_conv1d_glu_fwd", ctypes.byref(a), None if ws is None else ws.data_ptr(), mw, _s())
        Tout = T
        for i in range(a.nlayers):
            Tout = (Tout - 1) // 2 + 1
        Cg = a.cout[a.nlayers - 1] // 2
        out = arena[out_off:out_off + 2 * B * Tout * Cg].view(F16).view(B * Tout, Cg)
        return arena, out, bytes(a)

    def bwd(self, snap, arena, dy):
        """Backward of the forward whose argument snapshot is ``snap`` (weight / bias gradients)."""
        nb, _, sbytes, mw, sw = self.sizes(_lib.ConvArgs.from_buffer_copy(snap))
        dev = dy.device
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        if TransposedWeights.active is not None:
            TransposedWeights.active.wait_ready()
        main_ws = stream_workspace(mw, dev)
        side = 0
        if _Side.enabled:
            side_stream(dev)
            side = _Side.ptr
            with _SIDE_REGION:
                side_ws = _workspace("slab", sw, dev) if sw > 0 else None
        else:
            side_ws = _workspace("slab", sw, dev) if sw > 0 else None
        call("mms2ut_conv1d_glu_bwd", snap, dy.data_ptr(), scratch.data_ptr(),
             None if main_ws is None else main_ws.data_ptr(), mw, None if side_ws is None else side_ws.data_ptr(), sw,
             SIDE_WGRAD_BLOCKS if side else 0, _s(), side)
        if side:
            # the side stream reads the arena (im2col images) and the scratch (GLU gradients)
            _Side.keep.extend((arena, scratch, dy))
            _Side.used = True


def fusion_route(a):
    """Which form of the fusion attention the library takes for the argument block `a`
    (_lib.FusionArgs): 0 key-side, 1 query-side (include/mms2ut.h mms2ut_gated_fusion_route)."""
    r = _lib.load().mms2ut_gated_fusion_route(ctypes.byref(a))
    if r < 0:
        raise RuntimeError("mms2ut_gated_fusion_route: " + _lib.load().mms2ut_last_error().decode())
    return r


def fusion_set_route(mode):
    """Force a form of the fusion attention (tests, A/B runs): -1 by cost, 0 key-side, 1 query-side.
    Not to be changed between a forward and its backward."""
    call("mms2ut_gated_fusion_set_route", int(mode))


def fusion_pack_kv(Wkv, bkv, bias_kv, Dia):
    """[2d, Dia] = [Wkv | bkv | bias_kv (or 0) | 0...] (mms2ut_fusion_pack_kv)."""
    rows, Di = Wkv.shape
    assert Wkv.is_contiguous() and bkv.is_contiguous() and (bias_kv is None or bias_kv.is_contiguous())
    out = torch.empty(rows, Dia, dtype=F16, device=Wkv.device)
    call("mms2ut_fusion_pack_kv", Wkv.data_ptr(), bkv.data_ptr(), _p(bias_kv), out.data_ptr(), rows, Di, Dia, _s())
    return out


def fusion_unpack_kv(dw, gWkv, gbkv, g_bias_kv):
    """The inverse of fusion_pack_kv for the augmented weight gradient, on the side stream."""
    rows, Di = gWkv.shape
    assert gWkv.is_contiguous() and gbkv.is_contiguous() and dw.is_contiguous()
    ctx = side_begin(dw)
    with (ctx or _NULLCTX):
        call("mms2ut_fusion_unpack_kv", dw.data_ptr(), gWkv.data_ptr(), gbkv.data_ptr(), _p(g_bias_kv), rows, Di,
             dw.shape[1], _s())


class FusionCall:
    """The fusion tail (image LN, q / k|v projections, one-head attention, out-projection, sigmoid
    gate) enqueued by one library call each way (include/mms2ut.h mms2ut_gated_fusion_fwd / _bwd).
    Parameter / gradient / W^T pointers are bound once; each forward sets shapes, dropout sites and
    the arena and snapshots the argument block for its backward."""

    _sizes = {}

    def __init__(self, flags, params, grads, dgrad_weights):
        a = _lib.FusionArgs()
        for f, v in flags.items():
            setattr(a, f, v)
        for f, t in params.items():
            setattr(a, f, 0 if t is None else t.data_ptr())
        for f, t in grads.items():
            setattr(a, f, 0 if t is None else t.data_ptr())
        self.a = a
        self.dgrad_weights = dgrad_weights      # {"wt_q": W, ...}
        self.wt_of = None

    def _bind_wt(self):
        wt = TransposedWeights.active
        if wt is self.wt_of:
            return
        for f, W in self.dgrad_weights.items():
            img = wt.get(W, wait=False) if wt is not None else None
            setattr(self.a, f, 0 if img is None else img.data_ptr())
        self.wt_of = wt

    def route(self, B, Te, Ti):
        """The form the library takes at these shapes (fusion_route)."""
        a = self.a
        a.B, a.Te, a.Ti = B, Te, Ti
        return fusion_route(a)

    def sizes(self, want_dimg, a=None):
        """As ConvCall.sizes: `a` = a forward's argument snapshot (default: the live block)."""
        a = self.a if a is None else a
        key = (a.B, a.Te, a.Ti, a.Di, a.d, a.extra, a.gate, a.image_pre_norm, a.p_img > 0, a.p_txt > 0, a.p_attn > 0,
               bool(want_dimg), fusion_route(a))
        s = FusionCall._sizes.get(key)
        if s is None:
            oo, nb, sb, mw, sw = (ctypes.c_int64() for _ in range(5))
            so = (ctypes.c_int64 * 2)()
            call("mms2ut_gated_fusion_arena", ctypes.byref(a), ctypes.byref(oo), ctypes.byref(nb))
            call("mms2ut_gated_fusion_scratch", ctypes.byref(a), int(want_dimg), so, ctypes.byref(sb))
            call("mms2ut_gated_fusion_ws", ctypes.byref(a), ctypes.byref(mw), ctypes.byref(sw))
            s = (nb.value, oo.value, sb.value, list(so), mw.value, sw.value)
            FusionCall._sizes[key] = s
        return s

    def fwd(self, text, img, key_mask, B, Te, Ti, p, drops):
        """p = (p_img, p_txt, p_attn); drops = their (seed, offset) pairs or None.
        Returns (arena, output [B*Te, d] view, argument snapshot)."""
        a = self.a
        a.B, a.Te, a.Ti = B, Te, Ti
        a.p_img, a.p_txt, a.p_attn = p
        seeds = [dr[0] for dr in drops if dr is not None]
        a.seed = seeds[0] if seeds else 0
        assert all(sd == a.seed for sd in seeds), "one dropout seed per step"
        a.off_img, a.off_txt, a.off_attn = (dr[1] if dr is not None else 0 for dr in drops)
        a.key_mask, a.ld_mask = (key_mask.data_ptr(), key_mask.stride(0)) if key_mask is not None else (0, 0)
        a.text, a.img = text.data_ptr(), img.data_ptr()
        self._bind_wt()
        nb, oo, _, _, mw, _ = self.sizes(False)
        arena = torch.empty(nb, dtype=torch.uint8, device=text.device)
        a.saved = arena.data_ptr()
        ws = stream_workspace(mw, text.device)
        call("mms2ut_gated_fusion_fwd", ctypes.byref(a), None if ws is None else ws.data_ptr(), mw, _s())
        out = arena[oo:oo + 2 * B * Te * a.d].view(F16).view(B * Te, a.d)
        return arena, out, bytes(a)

    def bwd(self, snap, arena, keep, dres, want_dimg=False):
        """-> d(text) [B*Te, d] (and d(img) [B*Ti, Di] with want_dimg)."""
        a = _lib.FusionArgs.from_buffer_copy(snap)
        _, _, sbytes, so, mw, sw = self.sizes(want_dimg, a)
        dev = dres.device
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        if TransposedWeights.active is not None:
            TransposedWeights.active.wait_ready()
        main_ws = stream_workspace(mw, dev)
        side = 0
        if _Side.enabled:
            side_stream(dev)
            side = _Side.ptr
            with _SIDE_REGION:
                side_ws = _workspace("slab", sw, dev) if sw > 0 else None
        else:
            side_ws = _workspace("slab", sw, dev) if sw > 0 else None
        call("mms2ut_gated_fusion_bwd", snap, dres.data_ptr(), int(want_dimg), scratch.data_ptr(),
             None if main_ws is None else main_ws.data_ptr(), mw, None if side_ws is None else side_ws.data_ptr(), sw,
             SIDE_WGRAD_BLOCKS if side else 0, _s(), side)
        if side:
            _Side.keep.extend((arena, scratch, dres) + tuple(keep))
            _Side.used = True
        R, d = a.B * a.Te, a.d
        dtext = scratch[so[0]:so[0] + 2 * R * d].view(F16).view(R, d)
        if not want_dimg:
            return dtext
        Ri = a.B * a.Ti
        return dtext, scratch[so[1]:so[1] + 2 * Ri * a.Di].view(F16).view(Ri, a.Di)


def linear_dgrad(dy, W, out=None, *, epi=EPI_F16, aux=None, p=0.0, accumulate=False, drop=None):
    """dx[M,K] = dy[M,N] @ W[N,K]  (W row-major, reduction over N).  Reads the W^T image when one
    is registered (TransposedWeights), else W itself through transposed fragment reads.
    drop=(seed, offset): the forward dropout mask of the [M, K] output (EPI_GELU_DROP_BWD)."""
    M, N = dy.shape
    K = W.shape[1]
    if out is None:
        out = torch.empty(M, K, dtype=F16, device=dy.device)
    if accumulate:
        epi = EPI_F16_ACC
    seed, off = drop if (drop is not None and p > 0) else (0, 0)
    WT = TransposedWeights.active.get(W) if TransposedWeights.active is not None else None
    if WT is not None:
        gemm(dy, WT, out, M, K, N, a_kc=True, b_kc=True, lda=dy.stride(0), ldb=WT.stride(0),
             ldc=out.stride(0), epi=epi, aux=aux, ldaux=(aux.stride(0) if aux is not None else 0), p=p,
             seed=seed, offset=off, ld_rng=K)
        return out
    gemm(dy, W, out, M, K, N, a_kc=True, b_kc=False, lda=dy.stride(0), ldb=W.stride(0),
         ldc=out.stride(0), epi=epi, aux=aux, ldaux=(aux.stride(0) if aux is not None else 0), p=p,
         seed=seed, offset=off, ld_rng=K)
    return out


def _splitk_for(tiles, kred, slots=512):
    """split-K count for a weight gradient (reduction over kred token rows): the largest s whose
    tiles*s blocks still fit one round of the 512 block slots (2 per CU), so every block runs
    concurrently and no partial second round trails (round-2 scripts/wgrad_sweep.py, git history, isolated GEMM +
    slab reduction on the step's shapes: fc 3072x768 s3 vs the old fixed s8, qkv 2304x768 s4
    49 vs 60 us, cross-KV 9216x768 s1 174 vs 234 us; the 512-slot budget re-checked against
    256 / 1024 in round 2, profiles/round2_v3_wgrad_split_ab.txt).  Same rule as csrc/layers.hip."""
    s = max(1, min(16, slots // max(tiles, 1)))
    while s > 1 and kred // s < 256:
        s -= 1
    return s


class _Side:
    """Weight-gradient side stream: dW/db GEMMs and reductions do not feed the rest of the
    backward, so they run concurrently with the dgrad chain on a second HIP stream and fill the
    CUs the (latency-bound, dependent) dgrad kernels leave idle.

    The side region does not switch torch's current stream: kernels.py enqueues on
    ``override``.  Device memory read by side kernels (dy temporaries, saved activations) is kept
    referenced until ``side_join`` so the caching allocator cannot hand it to main-stream work
    before the side stream has consumed it; side-only scratch (split-K slabs, column partials)
    lives in persistent per-stream workspaces (the side stream serialises its own reuse)."""
    stream = None      # torch.cuda.Stream (RCCL buckets are enqueued on it, parallel.py)
    ptr = 0
    enabled = True     # False: side jobs run in order on the current stream (bench roofline pass)
    used = False
    override = 0
    keep = []
    ws = {}
    retain = False     # graph mode: regrown workspaces are retired, never freed (graphs bake pointers)
    retired = []


class _SideRegion:
    __slots__ = ()

    def __enter__(self):
        _Side.override = _Side.ptr
        return None

    def __exit__(self, *a):
        _Side.override = 0
        return False


_SIDE_REGION = _SideRegion()


class DevEvent:
    """A device-scope event (include/mms2ut.h mms2ut_event_*): orders work between this process's
    streams on one GPU without torch's system-scope fence (a full cache writeback per record,
    ~6 us of idle GPU each; profiles/round5_fork_fence.txt).  No timing, no host sync.  Owners
    re-record one event per use site; a wait binds to the record that precedes it."""
    __slots__ = ("h",)

    def __init__(self):
        h = ctypes.c_void_p()
        call("mms2ut_event_create", ctypes.addressof(h))
        self.h = h.value

    def record(self, stream):
        call("mms2ut_event_record", self.h, stream.cuda_stream)
        return self

    def wait(self, stream):
        call("mms2ut_event_wait", stream.cuda_stream, self.h)

    def __del__(self):
        try:
            if self.h:
                _lib.load().mms2ut_event_destroy(ctypes.c_void_p(self.h))
        except Exception:   # interpreter teardown
            pass


def stream_wait(waiter, signaler):
    """`waiter` waits for everything enqueued on `signaler` so far (device-scope event)."""
    if waiter.cuda_stream != signaler.cuda_stream:
        call("mms2ut_stream_wait", waiter.cuda_stream, signaler.cuda_stream)


_STREAMS = {}   # (device index, priority) -> ExternalStream, one per process


def make_stream(device, priority):
    """A non-blocking stream (include/mms2ut.h mms2ut_stream_create) wrapped for torch: work a
    caller leaves on the legacy NULL stream does not implicitly wait for it (measured equal to
    torch's pool streams in the bench, 17.05 vs 17.01-17.08 ms, round 4).  One stream per
    (device, priority) for the process: every Trainer reuses it, so building many trainers (test
    suites, tools) creates no more HIP streams (ExternalStream never destroys its handle; the cached
    ones are destroyed at exit, mms2ut_stream_destroy)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(priority))
    s = _STREAMS.get(key)
    if s is None:
        with torch.cuda.device(key[0]):
            h = ctypes.c_void_p()
            call("mms2ut_stream_create", int(priority), ctypes.addressof(h))
            s = torch.cuda.ExternalStream(h.value, device=dev)
        if not _STREAMS:
            atexit.register(_destroy_streams)
        _STREAMS[key] = s
    return s


def _destroy_streams():
    for s in _STREAMS.values():
        try:
            s.synchronize()
            _lib.load().mms2ut_stream_destroy(ctypes.c_void_p(s.cuda_stream))
        except Exception:   # interpreter teardown: the runtime may already be gone
            pass
    _STREAMS.clear()


def make_side_stream(device):
    """The weight-gradient side stream: lowest priority, so the hardware dispatcher prefers the
    critical path's workgroups (a CU-masked variant measured 5 % slower, round 1)."""
    return make_stream(device, 100)


def side_stream(device):
    """The (lazily created) weight-gradient side stream."""
    if _Side.stream is None:
        _Side.stream = make_side_stream(device)
        _Side.ptr = _Side.stream.cuda_stream
    return _Side.stream


def side_begin(*tensors):
    """Fork: the side stream waits for everything enqueued so far on the current stream."""
    if not _Side.enabled:
        return None
    if _Side.stream is None:
        _Side.stream = make_side_stream(_dev())
        _Side.ptr = _Side.stream.cuda_stream
    call("mms2ut_stream_wait", _Side.ptr, torch._C._cuda_getCurrentRawStream(_dev()))
    _Side.keep.extend(tensors)
    _Side.used = True
    return _SIDE_REGION


def wgrad_flush():
    """Launch a layer backward's deferred weight-gradient group now (mms2ut_wgrad_flush)."""
    call("mms2ut_wgrad_flush", torch._C._cuda_getCurrentRawStream(_dev()))


def side_join():
    """Join: the current stream waits for all side-stream work (before consuming gradients)."""
    if _Side.used and _Side.stream is not None:
        cur = torch._C._cuda_getCurrentRawStream(_dev())
        call("mms2ut_wgrad_flush", cur)   # a layer's deferred weight-gradient group, if any
        call("mms2ut_stream_wait", cur, _Side.ptr)
        _Side.used = False
        _Side.keep.clear()


def _workspace(key, numel, device, dtype=torch.float32):
    """Scratch owned by the stream it is used on (side-stream serialised reuse; regrowth keeps the
    old buffer alive until the next join)."""
    if _Side.override:
        buf = _Side.ws.get(key)
        if buf is None or buf.numel() < numel:
            if buf is not None:
                (_Side.retired if _Side.retain else _Side.keep).append(buf)
            buf = torch.empty(max(numel, 1 << 20), dtype=dtype, device=device)
            _Side.ws[key] = buf
        return buf[:numel]
    return torch.empty(numel, dtype=dtype, device=device)


class _nullctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULLCTX = _nullctx()


def _group_ok(dy, x, dW):
    N, K = dy.shape[1], x.shape[1]
    return (N % 8 == 0 and K % 8 == 0 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0 and
            dy.stride(1) == 1 and x.stride(1) == 1 and dW.is_contiguous() and
            all(t.data_ptr() % 16 == 0 for t in (dy, x, dW)) and
            dy.shape[0] * max(dy.stride(0), x.stride(0)) * 2 < 2 ** 31)


# grid cap of a grouped weight-gradient launch on the side stream (0: one block per tile).  A cap
# makes the launch persistent: 128 blocks held their slots for ~600 us per layer and pushed the
# critical path's 474-564-tile GEMMs into second rounds (22.4 ms per step against 18.1 uncapped
# or at 512, 18.5 with no side stream; profiles/round3_v1_side_blocks_ab.json).  Env
# MMS2UT_SIDE_WGRAD_BLOCKS overrides it (a multiple of 8; for A/B runs)
SIDE_WGRAD_BLOCKS = int(os.environ.get("MMS2UT_SIDE_WGRAD_BLOCKS", "0"))


def wgrad_group(problems, rows, max_blocks=0):
    """One grouped, unsplit weight-gradient launch (include/mms2ut.h mms2ut_wgrad_group):
    problems = [(dy [rows, N], x [rows, K], dW [N, K], db [N] or None), ...] (<= 8) on the current
    stream; dW / db overwritten; max_blocks > 0 caps the grid (persistent blocks)."""
    arr = (_lib.WgradArgs * len(problems))()
    for i, (dy, x, dW, db) in enumerate(problems):
        assert dy.shape[0] == rows and x.shape[0] == rows and tuple(dW.shape) == (dy.shape[1], x.shape[1])
        assert _group_ok(dy, x, dW), "wgrad_group: shapes / strides / alignment outside the kernel's rules"
        arr[i] = _lib.WgradArgs(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dW.data_ptr(),
                                0 if db is None else db.data_ptr(), dy.shape[1], x.shape[1])
    call("mms2ut_wgrad_group", arr, len(problems), int(rows), int(max_blocks), _s())


def linear_wgrad(dy, x, dW, *, db=None, accumulate_f32=None, out_f32=None, side=True):
    """dW[N,K] (fp16 view into the flat grad buffer) = dy[M,N]^T @ x[M,K].
    With accumulate_f32 (an fp32 [N,K] buffer) the result is added there instead; with out_f32 it
    is written there in fp32.
    With db (fp16 [N]) the bias gradient sum_rows dy comes out of the same GEMM: its first column
    of tiles sums the dy rows it stages anyway.  A product with >= 256 output tiles (one per CU)
    runs unsplit through the grouped kernel (no fp32 slabs); smaller ones split K over the rows
    into fp32 slabs, reduced by one launch."""
    M, N = dy.shape
    K = x.shape[1]
    assert dW is None or tuple(dW.shape) == (N, K)
    if out_f32 is not None:
        assert accumulate_f32 is None and db is None and tuple(out_f32.shape) == (N, K)
        accumulate_f32 = out_f32     # the split-K slab path below, its reduction storing (mode 0)
    if accumulate_f32 is None and -(-N // 128) * -(-K // 128) >= 256 and _group_ok(dy, x, dW):
        ctx = side_begin(dy, x) if side else None
        with (ctx or _NULLCTX):
            wgrad_group([(dy, x, dW, db)], M, SIDE_WGRAD_BLOCKS if ctx is not None and _Side.enabled else 0)
        return dW
    if db is not None and (accumulate_f32 is not None or K % 64 or N % 4):
        linear_wgrad(dy, x, dW, accumulate_f32=accumulate_f32, side=side)
        return bias_grad(dy, db, side=side)
    ctx = side_begin(dy, x) if side else None
    with (ctx or _NULLCTX):
        tiles = -(-N // 128) * -(-K // 128)
        s = _splitk_for(tiles, M)
        slabs = _workspace("slab", s * N * K, dy.device)
        rs = _workspace("rowsum", s * N, dy.device) if db is not None else None
        gemm(dy, x, slabs, N, K, M, a_kc=False, b_kc=False, lda=dy.stride(0), ldb=x.stride(0), ldc=K,
             epi=EPI_F32, splitk=s, sCsplit=N * K, rowsum=rs, ld_rowsum=N)
        if db is not None and accumulate_f32 is None and N % 4 == 0:
            call("mms2ut_splitk_reduce_bias", slabs.data_ptr(), s, N * K, N, K, dW.data_ptr(), dW.stride(0),
                 rs.data_ptr(), db.data_ptr(), _s())
            return dW
        if db is not None:
            call("mms2ut_splitk_reduce", rs.data_ptr(), s, N, 1, N, db.data_ptr(), N, 1, 1.0, _s())
        if accumulate_f32 is not None:
            call("mms2ut_splitk_reduce", slabs.data_ptr(), s, N * K, N, K, accumulate_f32.data_ptr(),
                 accumulate_f32.stride(0), 0 if out_f32 is not None else 2, 1.0, _s())
            return accumulate_f32
        call("mms2ut_splitk_reduce", slabs.data_ptr(), s, N * K, N, K, dW.data_ptr(), dW.stride(0), 1,
             1.0, _s())
    return dW


def bias_grad(dy, db, accumulate=False, side=True):
    """db[N] = sum_rows dy[M,N] (fp16 out, fp32 accumulation)."""
    M, N = dy.shape
    L = _lib.load()
    ctx = side_begin(dy) if side else None
    with (ctx or _NULLCTX):
        nparts = L.mms2ut_colsum_nparts(M)
        part = _workspace("colsum", nparts * N, dy.device)
        call("mms2ut_colsum_f16", dy.data_ptr(), M, N, dy.stride(0), part.data_ptr(), nparts, _s())
        call("mms2ut_colsum_parts", part.data_ptr(), nparts, N, db.data_ptr(), int(accumulate), _s())
    return db

# ============================================================================ LayerNorm


def layernorm(x, g, b, eps=1e-5, *, out=None, grp=0, grp_out=0, p=0.0, drop=None):
    """y = LN(x).  With out/grp/grp_out/p the result goes to row (r // grp) * grp_out + r % grp of
    out (a padded layout) after dropout_p with the unpadded counters (layernorm_fwd_ex)."""
    R, D = x.shape
    mean = torch.empty(R, dtype=torch.float32, device=x.device)
    rstd = torch.empty(R, dtype=torch.float32, device=x.device)
    if out is None and not grp and p == 0.0:
        y = torch.empty_like(x)
        call("mms2ut_layernorm_fwd", x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(),
             mean.data_ptr(), rstd.data_ptr(), R, D, eps, _s())
        return y, mean, rstd
    y = torch.empty_like(x) if out is None else out
    assert y.is_contiguous() and y.shape[-1] == D
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_layernorm_fwd_ex", x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(),
         mean.data_ptr(), rstd.data_ptr(), R, D, eps, int(grp), int(grp_out), float(p), seed, off, _s())
    return y, mean, rstd


def layernorm_bwd(dy, x, g, mean, rstd, dgb, dres=None, want_dx=True, emit=None, dy_grp=0, dy_grp_out=0,
                  dy_p=0.0, dy_drop=None, dgb_accumulate=False):
    """Returns dx (+dres). dgb: fp16 view of [dgamma | dbeta] (2*D contiguous), overwritten, or
    added to with dgb_accumulate (one LayerNorm applied at several places).
    emit=(p, (seed, offset)): also return dropout(dx) for the sublayer below -> (dx, dxd).
    dy_grp/dy_grp_out/dy_p: dy is read through layernorm(out=, grp=, p=)'s layout and dropout."""
    R, D = x.shape
    if dy_grp or dy_p > 0:
        assert emit is None and D % 256 == 0 and D <= 1024
        L = _lib.load()
        nparts = L.mms2ut_layernorm_bwd_nparts(R, D)
        part = torch.empty(nparts, 2 * D, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if want_dx else None
        seed, off = dy_drop if dy_p > 0 else (0, 0)
        call("mms2ut_layernorm_bwd_ex", dy.data_ptr(), x.data_ptr(), g.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), _p(dres), _p(dx), part.data_ptr(), R, D, None, 0.0, 0, 0, int(dy_grp),
             int(dy_grp_out), float(dy_p), seed, off, _s())
        ctx = side_begin(part)
        with (ctx or _NULLCTX):
            call("mms2ut_colsum_parts", part.data_ptr(), nparts, 2 * D, dgb.data_ptr(), 0, _s())
        return dx
    L = _lib.load()
    nparts = L.mms2ut_layernorm_bwd_nparts(R, D)
    part = torch.empty(nparts, 2 * D, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_dx else None
    dxd, p, seed, off = None, 0.0, 0, 0
    if emit is not None and emit[0] > 0:
        p, (seed, off) = emit
        dxd = torch.empty_like(x)
    call("mms2ut_layernorm_bwd", dy.data_ptr(), x.data_ptr(), g.data_ptr(), mean.data_ptr(),
         rstd.data_ptr(), _p(dres), _p(dx), part.data_ptr(), R, D, _p(dxd), float(p), seed, off, _s())
    # gamma/beta gradients feed only the optimizer: their partial-sum reduction leaves the
    # critical path for the weight-gradient side stream
    ctx = side_begin(part)
    with (ctx or _NULLCTX):
        call("mms2ut_colsum_parts", part.data_ptr(), nparts, 2 * D, dgb.data_ptr(), int(dgb_accumulate), _s())
    if emit is not None:
        return dx, (dxd if dxd is not None else dx)
    return dx

# ============================================================================ attention


def attn_softmax(S, Z, H, Tq, Tk, ldS, key_len=None, key_mask=None, causal=False, extra_key=False,
                 p=0.0, drop=None):
    P = torch.empty_like(S)
    Pd = torch.empty_like(S) if p > 0 else P
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_attn_softmax_fwd", S.data_ptr(), P.data_ptr(), Pd.data_ptr(), Z, H, Tq, Tk, ldS,
         _p(key_len), _p(key_mask), (key_mask.stride(0) if key_mask is not None else 0),
         int(causal), int(extra_key), float(p), seed, off, _s())
    return P, Pd


def attn_softmax_bwd(P, dPd, Z, H, Tq, Tk, ldS, p=0.0, drop=None, out=None):
    seed, off = drop if p > 0 else (0, 0)
    dS = dPd if out is None else out
    call("mms2ut_attn_softmax_bwd", P.data_ptr(), dPd.data_ptr(), dS.data_ptr(), Z, H, Tq, Tk, ldS,
         None, 0, 0, float(p), seed, off, _s())
    return dS

def attn_softmax_aug(S, Z, Tq, Tk, ldS, q_aug, scale, n_img, u_aug, npad, key_mask=None, extra_key=False,
                     p=0.0, drop=None):
    """attn_softmax (H = 1) with the query-side fusion attention's tail columns
    (mms2ut_attn_softmax_fwd_aug): q_aug / u_aug are column views [rows, >= 2 / npad]."""
    P = torch.empty_like(S)
    Pd = torch.empty_like(S) if p > 0 else P
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_attn_softmax_fwd_aug", S.data_ptr(), P.data_ptr(), Pd.data_ptr(), Z, Tq, Tk, ldS,
         _p(key_mask), (key_mask.stride(0) if key_mask is not None else 0), int(extra_key), float(p), seed, off,
         q_aug.data_ptr(), q_aug.stride(0), float(scale), int(n_img), u_aug.data_ptr(), u_aug.stride(0), int(npad),
         _s())
    return P, Pd


def attn_softmax_bwd_aug(P, dPd, Z, Tq, Tk, ldS, du_aug, scale, n_img, dq_aug, npad, p=0.0, drop=None):
    """attn_softmax_bwd in place with the tail columns (mms2ut_attn_softmax_bwd_aug)."""
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_attn_softmax_bwd_aug", P.data_ptr(), dPd.data_ptr(), dPd.data_ptr(), Z, Tq, Tk, ldS, float(p),
         seed, off, du_aug.data_ptr(), du_aug.stride(0), float(scale), int(n_img), dq_aug.data_ptr(),
         dq_aug.stride(0), int(npad), _s())
    return dPd

FLASH_HD = (64, 96, 128)


def _attn_args(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
               sq=0, sk=0, sv=0, so=0):
    """mms2ut_attn_args packed in one struct call (_lib.ATTN_ARGS, fields in AttnArgs order)."""
    seed, off = drop if p > 0 else (0, 0)
    return _lib.ATTN_ARGS.pack(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo,
                               sq, sk, sv, so, B, H, Tq, Tk, hd, 0 if key_len is None else key_len.data_ptr(),
                               int(causal), scale, p, seed, off, 0 if lse is None else lse.data_ptr())


def _plan_dict(plan):
    return {n: int(getattr(plan, n)) for n, _ in plan._fields_}


def mha_fwd(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len=None, causal=False,
            p=0.0, drop=None, sq=0, sk=0, sv=0, so=0):
    """Fused attention forward; returns the row log-sum-exp [B*H*Tq] (fp32) for the backward.
    s*: batch strides in elements (0 = rows of one batch follow each other: T * ld)."""
    lse = torch.empty(B * H * Tq, dtype=torch.float32, device=q.device)
    a = _attn_args(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
                   sq, sk, sv, so)
    call("mms2ut_mha_varlen_fwd", a, _s())
    return lse


def mha_fwd_plan(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len=None, causal=False,
                 p=0.0, drop=None, sq=0, sk=0, sv=0, so=0):
    """What mha_fwd would launch for these arguments (mms2ut_mha_varlen_fwd_plan; host only):
    {nw, short_k, grid_x, grid_y}.  Raises as mha_fwd would on arguments it rejects."""
    lse = torch.empty(1, dtype=torch.float32, device=q.device)   # only its presence is looked at
    a = _attn_args(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
                   sq, sk, sv, so)
    plan = _lib.AttnFwdPlan()
    call("mms2ut_mha_varlen_fwd_plan", a, ctypes.addressof(plan))
    return _plan_dict(plan)


def mha_bwd(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
            dout, lddo, dq, lddq, dk, lddk, dv, lddv, sq=0, sk=0, sv=0, so=0, sdo=0, sdq=0, sdk=0, sdv=0):
    """Fused attention backward: dq / dk / dv written.  s*: batch strides in elements as in mha_fwd."""
    a = _attn_args(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
                   sq, sk, sv, so)
    Dd = torch.empty(B * H * Tq, dtype=torch.float32, device=q.device)
    call("mms2ut_mha_varlen_bwd", a, dout.data_ptr(), int(lddo), int(sdo), Dd.data_ptr(), dq.data_ptr(),
         int(lddq), int(sdq), dk.data_ptr(), int(lddk), int(sdk), dv.data_ptr(), int(lddv), int(sdv), _s())


def mha_bwd_plan(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
                 dout, lddo, dq, lddq, dk, lddk, dv, lddv, sq=0, sk=0, sv=0, so=0, sdo=0, sdq=0, sdk=0, sdv=0):
    """What mha_bwd would launch for these arguments (mms2ut_mha_varlen_bwd_plan; host only):
    {fused, nkc, kv16, rows_prep, grid, rounds}.  Raises as mha_bwd would on arguments it rejects."""
    a = _attn_args(q, k, v, o, ldq, ldk, ldv, ldo, B, H, Tq, Tk, hd, scale, key_len, causal, p, drop, lse,
                   sq, sk, sv, so)
    plan = _lib.AttnBwdPlan()
    Dd = torch.empty(1, dtype=torch.float32, device=q.device)    # only its presence is looked at
    call("mms2ut_mha_varlen_bwd_plan", a, dout.data_ptr(), int(lddo), int(sdo), Dd.data_ptr(), dq.data_ptr(),
         int(lddq), int(sdq), dk.data_ptr(), int(lddk), int(sdk), dv.data_ptr(), int(lddv), int(sdv),
         ctypes.addressof(plan))
    return _plan_dict(plan)

# ============================================================================ elementwise


def dropout(x, p, drop, out=None):
    out = x if out is None else out
    if p <= 0:
        if out.data_ptr() != x.data_ptr():
            out.copy_(x)
        return out
    seed, off = drop
    call("mms2ut_dropout_fwd", x.data_ptr(), out.data_ptr(), x.numel(), float(p), seed, off, _s())
    return out


def dropout_mask(n, p, seed, offset, device):
    m = torch.empty(n, dtype=torch.uint8, device=device)
    call("mms2ut_dropout_mask", m.data_ptr(), n, float(p), int(seed), int(offset), _s())
    return m


def encoder_embed(h, pos_table, lens32, B, T, D, scale, p, drop):
    x = torch.empty_like(h)
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_encoder_embed_fwd", h.data_ptr(), pos_table.data_ptr(), lens32.data_ptr(),
         x.data_ptr(), B, T, D, float(scale), float(p), seed, off, _s())
    return x


def scale_dropout_bwd(dx, scale, p, drop, out=None):
    out = torch.empty_like(dx) if out is None else out
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_scale_dropout_bwd", dx.data_ptr(), out.data_ptr(), dx.numel(), float(scale),
         float(p), seed, off, _s())
    return out


def token_embed(tok, E, pos_table, B, T, D, pad, scale, p, drop):
    x = torch.empty(B * T, D, dtype=F16, device=E.device)
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_token_embed_fwd", tok.data_ptr(), E.data_ptr(), pos_table.data_ptr(), x.data_ptr(),
         B, T, D, pad, float(scale), float(p), seed, off, _s())
    return x


def token_embed_bwd(tok, dx, dE32, B, T, D, pad, scale, p, drop):
    seed, off = drop if p > 0 else (0, 0)
    call("mms2ut_token_embed_bwd", tok.data_ptr(), dx.data_ptr(), dE32.data_ptr(), B, T, D, dE32.shape[0], pad,
         float(scale), float(p), seed, off, _s())


def add_f32_to_f16(a, b32, out):
    call("mms2ut_add_f32_to_f16", a.data_ptr(), b32.data_ptr(), out.data_ptr(), a.numel(), _s())
    return out


def add_f16(a, b, out=None):
    out = torch.empty_like(a) if out is None else out
    call("mms2ut_add_f16", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _s())
    return out


def glu(x, C):
    rows = x.shape[0]
    y = torch.empty(rows, C, dtype=F16, device=x.device)
    call("mms2ut_glu_fwd", x.data_ptr(), y.data_ptr(), rows, C, _s())
    return y


def glu_bwd(x, dy, C):
    rows = x.shape[0]
    dx = torch.empty(rows, 2 * C, dtype=F16, device=x.device)
    call("mms2ut_glu_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), rows, C, _s())
    return dx


def im2col(x, B, Tin, Tout, C, k, stride=2, pad=None, ldcol=None):
    """col [B*Tout, ldcol] (ldcol >= C*k, zero columns past C*k)."""
    pad = k // 2 if pad is None else pad
    ldcol = C * k if ldcol is None else ldcol
    col = torch.empty(B * Tout, ldcol, dtype=F16, device=x.device)
    call("mms2ut_im2col_ld", x.data_ptr(), col.data_ptr(), B, Tin, Tout, C, k, stride, pad, ldcol, _s())
    return col


def col2im(dcol, B, Tin, Tout, C, k, stride=2, pad=None):
    pad = k // 2 if pad is None else pad
    dx = torch.empty(B * Tin, C, dtype=F16, device=dcol.device)
    call("mms2ut_col2im", dcol.data_ptr(), dx.data_ptr(), B, Tin, Tout, C, k, stride, pad, _s())
    return dx


def gate_bwd(dres, merge, g):
    R, D = dres.shape
    dpre = torch.empty_like(dres)
    dmerge = torch.empty(R, 2 * D, dtype=F16, device=dres.device)
    call("mms2ut_gate_bwd", dres.data_ptr(), merge.data_ptr(), g.data_ptr(), dpre.data_ptr(),
         dmerge.data_ptr(), R, D, _s())
    return dpre, dmerge


def copy2d(src, dst, rows, cols):
    call("mms2ut_copy2d", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols,
         _s())

# ============================================================================ loss / optimizer


LS_XENT_PARTS = 512   # include/mms2ut.h MMS_LS_XENT_PARTS


def ls_xent_fwd(logits, ld, target, rows, V, eps, pad, loss_out, call_out=None):
    """loss_out[0:2] += {label-smoothed loss, nll} (fixed-order sum; loss_out may be None) and, with
    call_out, call_out[0:2] = this call's {loss, nll}; returns lse [rows]."""
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    part = _workspace("ls_xent_part", 2 * LS_XENT_PARTS, logits.device)
    call("mms2ut_ls_xent_fwd_log", logits.data_ptr(), ld, target.data_ptr(), rows, V, float(eps), pad,
         lse.data_ptr(), part.data_ptr(), _p(loss_out), _p(call_out), _s())
    return lse


EVAL_LOSS, EVAL_NLL, EVAL_NTOKENS, EVAL_NCORRECT = range(4)


def ls_xent_eval(logits, ld, target, rows, V, eps, pad, stats):
    """Validation scoring, forward only: stats (fp64 device [4]) += {label-smoothed loss, nll,
    non-pad targets, rows whose argmax over [0, V) is the target}.  Accumulates over calls (the
    caller zeroes ``stats`` once per split); no host sync."""
    assert stats.dtype == torch.float64 and stats.numel() == 4 and stats.is_contiguous()
    _chk(logits)
    _chk(target, torch.int64)
    assert stats.is_cuda and target.numel() >= rows and logits.numel() >= rows * ld
    part = _workspace("ls_xent_eval_part", 4 * LS_XENT_PARTS, logits.device, torch.float64)
    call("mms2ut_ls_xent_eval", logits.data_ptr(), ld, target.data_ptr(), rows, V, float(eps), pad,
         part.data_ptr(), stats.data_ptr(), _s())
    return stats


def set_f32(dst, vals):
    """dst[:len(vals)] = vals (fp32 device vector, <= 8 values) in one launch."""
    import ctypes
    arr = (ctypes.c_float * len(vals))(*[float(v) for v in vals])
    call("mms2ut_set_f32", dst.data_ptr(), len(vals), ctypes.addressof(arr), _s())


def ls_xent_bwd(logits, ld, target, rows, V, eps, pad, lse, grad, out):
    call("mms2ut_ls_xent_bwd", logits.data_ptr(), ld, target.data_ptr(), rows, V, float(eps), pad,
         lse.data_ptr(), grad.data_ptr(), out.data_ptr(), _s())
    return out


def ls_xent_rdrop_fwd(logits, ld, target, rows, V, eps, pad, alpha, acc=None, acc_kl=None, call_out=None):
    """R-Drop forward over logits [rows = 2R, ld] (two dropout passes, row r pairs with row r + R)
    and the first half's targets [R]: acc[0:2] += {CE over 2R rows + alpha * kl, nll},
    acc_kl[0] += kl, call_out[0:3] = this call's {loss, nll, kl} (fixed-order sums; each may be
    None, not all); returns lse [rows] (0 on pad pairs)."""
    _chk(logits)
    _chk(target, torch.int64)
    assert target.numel() >= rows // 2 and logits.numel() >= rows * ld
    lse = torch.empty(max(rows, 1), dtype=torch.float32, device=logits.device)[:rows]
    part = _workspace("ls_xent_rdrop_part", 3 * LS_XENT_PARTS, logits.device)
    call("mms2ut_ls_xent_rdrop_fwd", logits.data_ptr(), ld, target.data_ptr(), rows, V, float(eps), pad,
         float(alpha), lse.data_ptr(), part.data_ptr(), _p(acc), _p(acc_kl), _p(call_out), _s())
    return lse


def ls_xent_rdrop_bwd(logits, ld, target, rows, V, eps, pad, alpha, lse, grad, out):
    """out (may be ``logits``) = grad * [(p - y_smooth) + alpha * dkl/dz] for both halves."""
    call("mms2ut_ls_xent_rdrop_bwd", logits.data_ptr(), ld, target.data_ptr(), rows, V, float(eps), pad,
         float(alpha), lse.data_ptr(), grad.data_ptr(), out.data_ptr(), _s())
    return out


OST_MULT, OST_GNORM, OST_OVERFLOW, OST_STEP, OST_STEP_SIZE, OST_LOSS_SCALE, OST_ITER, \
    OST_LAST_OVERFLOW, OST_LAST_RESCALE, OST_CLIP_COEF, OST_FATAL, OST_LR, OST_INCONSISTENT = range(13)
OST_SIZE = 16


def grad_norm(grad, ost, sample_size=None, nparts=1024):
    part = torch.empty(nparts, dtype=torch.float32, device=grad.device)
    call("mms2ut_grad_sqnorm", grad.data_ptr(), grad.numel(), part.data_ptr(), nparts, _s())
    call("mms2ut_grad_norm_finalize", part.data_ptr(), nparts, ost.data_ptr(), _p(sample_size), _s())


def ctc_loss_fwd(logits, B, T, V, targets, in_len32, tgt_len32, max_tgt_len, blank, zero_infinity, loss_sum):
    """Adds the summed CTC loss to loss_sum (fp32 [1]); returns the workspace for ctc_loss_bwd."""
    import ctypes
    n = ctypes.c_int64()
    call("mms2ut_ctc_workspace_floats", int(B), int(T), int(max_tgt_len), ctypes.byref(n))
    work = torch.empty(max(n.value, 1), dtype=torch.float32, device=logits.device)
    assert targets.dtype == torch.int64 and in_len32.dtype == torch.int32 and tgt_len32.dtype == torch.int32
    call("mms2ut_ctc_loss_fwd", logits.data_ptr(), logits.stride(0), int(B), int(T), int(V), targets.data_ptr(),
         targets.stride(0), int(max_tgt_len), in_len32.data_ptr(), tgt_len32.data_ptr(), int(blank),
         int(zero_infinity), work.data_ptr(), loss_sum.data_ptr(), _s())
    return work


def ctc_loss_bwd(logits, B, T, V, targets, in_len32, tgt_len32, max_tgt_len, blank, work, grad_scale, out=None):
    out = torch.empty_like(logits) if out is None else out
    call("mms2ut_ctc_loss_bwd", logits.data_ptr(), logits.stride(0), int(B), int(T), int(V), targets.data_ptr(),
         targets.stride(0), int(max_tgt_len), in_len32.data_ptr(), tgt_len32.data_ptr(), int(blank), work.data_ptr(),
         grad_scale.data_ptr(), out.data_ptr(), out.stride(0), _s())
    return out


def grad_norm_check(buf, world, rank, ost, stage):
    call("mms2ut_grad_norm_check", buf.data_ptr(), int(world), int(rank), ost.data_ptr(), int(stage), _s())


def scale_f16(x, alpha):
    call("mms2ut_scale_f16", x.data_ptr(), x.numel(), float(alpha), _s())
    return x


_bound_seed = [None]


def bind_step_seed(delta):
    """Bind (or with None unbind) the device step-seed delta every dropout kernel adds to its seed
    (graph replay; include/mms2ut.h mms2ut_bind_step_seed).  Process-global; rebinding the bound
    tensor is free."""
    if delta is _bound_seed[0]:
        return
    if delta is not None:
        assert delta.is_cuda and delta.dtype == torch.int64 and delta.numel() == 1
    call("mms2ut_bind_step_seed", None if delta is None else delta.data_ptr())
    _bound_seed[0] = delta


def step_seed_advance(delta, inc):
    call("mms2ut_step_seed_advance", delta.data_ptr(), int(inc) & ((1 << 64) - 1), _s())


def accum_f16_f32(acc, x):
    assert acc.dtype == torch.float32 and x.dtype == F16 and acc.numel() == x.numel()
    call("mms2ut_accum_f16_f32", acc.data_ptr(), x.data_ptr(), x.numel(), _s())
    return acc


def optim_prepare(ost, lr, warmup_init_lr, warmup_updates, beta1, beta2, clip, scale_window, min_scale):
    call("mms2ut_optim_prepare", ost.data_ptr(), float(lr), float(warmup_init_lr), float(warmup_updates),
         float(beta1), float(beta2), float(clip), float(scale_window), float(min_scale), _s())


def adam(param, grad, master, m, v, ost, beta1, beta2, eps, wd):
    call("mms2ut_adam_fp16_master", param.data_ptr(), grad.data_ptr(), master.data_ptr(),
         m.data_ptr(), v.data_ptr(), param.numel(), ost.data_ptr(), float(beta1),
         float(beta2), float(eps), float(wd), _s())

# ============================================================================ fbank


def fbank(wave, wave_off, frame_off, total_frames, banks, mel_range, nbins=80):
    feats = torch.empty(total_frames, nbins, dtype=torch.float32, device=wave.device)
    B = wave_off.numel() - 1
    call("mms2ut_fbank_f32", wave.data_ptr(), wave_off.data_ptr(), frame_off.data_ptr(), B,
         total_frames, banks.data_ptr(), mel_range.data_ptr(), nbins, feats.data_ptr(), _s())
    return feats


CMVN_SPLIT = 8   # include/mms2ut.h MMS_CMVN_SPLIT


def cmvn_collate(feats, frame_off, B, Tmax, nbins=80, cmvn=True):
    out = torch.empty(B, Tmax, nbins, dtype=F16, device=feats.device)
    # include/mms2ut.h MMS_CMVN_WS_FLOATS: fp32 stats, then fp64 slice partials
    stats = torch.empty(((2 * B * nbins + 1) & ~1) + 2 * B * CMVN_SPLIT * 2 * nbins, dtype=torch.float32,
                        device=feats.device)
    call("mms2ut_fbank_cmvn_collate", feats.data_ptr(), frame_off.data_ptr(), B, Tmax, nbins,
         int(cmvn), stats.data_ptr(), out.data_ptr(), _s())
    return out


def specaugment(x, frame_off, masks, n_freq, n_time, mask_value=None):
    """In place on collated fp16 features x [B, Tmax, nbins]; masks int32 [B, 2*(n_freq+n_time)]
    on x's device (see include/mms2ut.h)."""
    B, Tmax, nbins = x.shape
    if masks.shape != (B, 2 * (n_freq + n_time)) or masks.dtype != torch.int32 or masks.device != x.device:
        raise ValueError(f"specaugment: masks {tuple(masks.shape)} {masks.dtype} for B={B}, {n_freq}+{n_time} masks")
    call("mms2ut_specaugment_f16", x.data_ptr(), frame_off.data_ptr(), B, Tmax, nbins, masks.data_ptr(),
         int(n_freq), int(n_time), int(mask_value is not None), float(mask_value or 0.0), _s())
    return x


NOISE_SPLIT, NOISE_MAX_MIX = 8, 4   # include/mms2ut.h MMS_NOISE_SPLIT, MMS_NOISE_MAX_MIX


def noise_mix(wb, bank, bank_off, params, n_mix):
    """Noise augmentation in place on the wave batch ``wb`` (FbankFrontend.upload / from_device):
    bank int16 [N] + bank_off int64 [n_clips + 1] and params int32 [B, 3 + n_mix] on the wave's
    device (see include/mms2ut.h; the caller has validated params, frontend.NoiseAugment.check)."""
    wave, B = wb["wave"], wb["B"]
    if not 1 <= n_mix <= NOISE_MAX_MIX:
        raise ValueError(f"noise_mix: n_mix {n_mix} (1 .. {NOISE_MAX_MIX})")
    if params.shape != (B, 3 + n_mix) or params.dtype != torch.int32 or params.device != wave.device \
            or not params.is_contiguous():
        raise ValueError(f"noise_mix: params {tuple(params.shape)} {params.dtype} for B={B}, n_mix={n_mix}")
    if bank.dtype != torch.int16 or bank_off.dtype != torch.int64 or bank.device != wave.device \
            or bank_off.device != wave.device or wave.dtype != torch.float32:
        raise ValueError("noise_mix: int16 bank, int64 offsets and fp32 wave on one device expected")
    ws = torch.empty(3 * B * NOISE_SPLIT, dtype=torch.float64, device=wave.device)   # MMS_NOISE_WS_DOUBLES
    call("mms2ut_noise_mix_f32", wave.data_ptr(), wb["wave_off"].data_ptr(), B, bank.data_ptr(),
         bank_off.data_ptr(), bank_off.numel() - 1, params.data_ptr(), int(n_mix), ws.data_ptr(), _s())
    return wave


RESAMPLE_TILE, RESAMPLE_MAX_TAPS = 2048, 1 << 20   # include/mms2ut.h MMS_RESAMPLE_TILE, MMS_RESAMPLE_MAX_TAPS


def resample_tile(o, n, K):
    """Outputs one block of mms2ut_resample_f32 owns for this filter: whole frames of n outputs, about
    RESAMPLE_TILE of them, fewer where the input window would not fit in LDS (include/mms2ut.h
    mms2ut_resample_plan).  Raises for a table over RESAMPLE_MAX_TAPS.  Needs no device."""
    f = _lib.C.c_int(0)
    call("mms2ut_resample_plan", int(o), int(n), int(K), _lib.C.byref(f))
    return f.value * int(n)


def resample(x, in_off, taps, o, n, width, int16=False):
    """Polyphase sinc resampling (include/mms2ut.h mms2ut_resample_f32) of mono fp32 clips laid back to
    back in x; in_off: int64 [B + 1] sample offsets on the host (numpy or CPU tensor), every clip
    non-empty; taps: fp32 [K, n] on x's device, tap-major (prepare.resample_taps(...)[0].T).
    -> (y fp32 [total], out_off int64 numpy [B + 1], y16 int16 [total] or None); clip b of L samples owns
    y[out_off[b]:out_off[b + 1]], ceil(n L / o) samples."""
    import numpy as np
    in_off = np.asarray(in_off, dtype=np.int64).reshape(-1)
    o, n, width = int(o), int(n), int(width)
    K = 2 * width + o
    if o < 1 or n < 1 or width < 0 or math.gcd(o, n) != 1:
        raise ValueError(f"resample: o {o}, n {n} must be coprime and >= 1, width {width} >= 0")
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"resample: contiguous 1-D fp32 device samples expected, got {tuple(x.shape)} {x.dtype}")
    if taps.shape != (K, n) or taps.dtype != torch.float32 or taps.device != x.device or not taps.is_contiguous():
        raise ValueError(f"resample: taps {tuple(taps.shape)} {taps.dtype} for K={K}, n={n} (tap-major fp32 on "
                         f"{x.device} expected)")
    if in_off.size < 1 or in_off[0] != 0 or in_off[-1] != x.numel():
        raise ValueError(f"resample: in_off must run from 0 to {x.numel()} samples")
    lens = np.diff(in_off)
    if (lens <= 0).any():
        raise ValueError("resample: empty clip")
    resample_tile(o, n, K)                      # the table cap and the LDS window, before anything is allocated
    out_lens = (lens * n + o - 1) // o
    out_off = np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64)
    B, total = int(lens.size), int(out_off[-1])
    y = torch.empty(total, dtype=torch.float32, device=x.device)
    y16 = torch.empty(total, dtype=torch.int16, device=x.device) if int16 else None
    if B:
        offs = torch.from_numpy(np.stack([in_off, out_off])).to(x.device)
        call("mms2ut_resample_f32", x.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), B, int(out_lens.max()),
             taps.data_ptr(), o, n, width, K, y.data_ptr(), _p(y16), _s())
    return y, out_off, y16


def log_softmax_step(logits, V, pad, eos, mode=0, out=None):
    """fp32 [rows, V] = log_softmax(logits[:, :V].float()) with the beam-search step masks
    (mode 0: pad; 1: force eos; 2: forbid eos)."""
    rows = logits.shape[0]
    out = torch.empty(rows, V, dtype=torch.float32, device=logits.device) if out is None else out
    call("mms2ut_log_softmax_step", logits.data_ptr(), logits.stride(0), rows, int(V), int(pad), int(eos),
         int(mode), out.data_ptr(), _s())
    return out


UNK = 3                    # fairseq Dictionary: <s> 0, <pad> 1, </s> 2, <unk> 3
SAMPLE_MAX_V = 4096        # sample_step keeps one row's (lprob, index) pairs in LDS
SAMPLE_MAX_BEAM = 256      # the draw's slot takes 8 bits of the stream's counter


def log_softmax_step_ext(logits, V, pad, eos, mode=0, temperature=1.0, unk_penalty=0.0, unk=UNK, out=None):
    """log_softmax_step with --temperature (logit = fp16(float(z) / T)) and --unkpen (subtracted
    from column ``unk`` between the pad mask and the eos masks).  T = 1, unkpen = 0 is
    log_softmax_step bit for bit."""
    if not temperature > 0:
        raise ValueError(f"log_softmax_step_ext: temperature must be greater than 0, got {temperature}")
    if logits.dtype != F16 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V:
        raise ValueError(f"log_softmax_step_ext: logits must be fp16 [rows, >= {V}] with unit column stride, got "
                         f"{logits.dtype} {tuple(logits.shape)}")
    rows = logits.shape[0]
    out = torch.empty(rows, V, dtype=torch.float32, device=logits.device) if out is None else out
    call("mms2ut_log_softmax_step_ext", logits.data_ptr(), logits.stride(0), rows, int(V), int(pad), int(eos),
         int(unk), int(mode), float(temperature), float(unk_penalty), out.data_ptr(), _s())
    return out


def ngram_block(tokens, lprobs, step, n):
    """--no-repeat-ngram-size n on lprobs [N, V] fp32 in place (mms2ut_ngram_block): tokens [N, ld]
    int64 are the histories, columns [0, step] filled.  Returns lprobs."""
    N, V = lprobs.shape
    if tokens.dtype != torch.int64 or tokens.dim() != 2 or tokens.shape[0] != N or not tokens.is_contiguous() \
            or lprobs.dtype != torch.float32 or not lprobs.is_contiguous() or tokens.device != lprobs.device:
        raise ValueError(f"ngram_block: expected contiguous int64 tokens [{N}, ld] and fp32 lprobs [{N}, {V}] on one "
                         f"device, got {tokens.dtype} {tuple(tokens.shape)} and {lprobs.dtype} {tuple(lprobs.shape)}")
    if not 0 <= step < tokens.shape[1]:
        raise ValueError(f"ngram_block: step {step} outside the histories' {tokens.shape[1]} columns")
    if n < 1 or n > 64:
        raise ValueError(f"ngram_block: n must be in [1, 64], got {n}")
    call("mms2ut_ngram_block", tokens.data_ptr(), tokens.shape[1], N, int(step), int(n), lprobs.data_ptr(), V, _s())
    return lprobs


def sample_step(lprobs, prev_col, ids, bsz, beam, V, step, seed, topk=-1, topp=-1.0, first_step=None):
    """fairseq Sampling.step (mms2ut_sample_step) -> (scores, tokens, beams [bsz, beam], lprob
    [bsz, beam] f32 the drawn token's own lprob, kept [bsz, beam] i32 the size of the set drawn
    from).  lprobs [bsz*beam, V] fp32, prev_col a strided fp32 column [bsz*beam] of the cumulative
    scores (None at the first step), ids int64 [bsz] the sentences' ids (the stream's key)."""
    first_step = step == 0 if first_step is None else first_step
    if V > SAMPLE_MAX_V:
        raise NotImplementedError(f"sample_step: vocabulary {V} exceeds the kernel's limit of {SAMPLE_MAX_V}")
    if beam > SAMPLE_MAX_BEAM:
        raise ValueError(f"sample_step: beam {beam} exceeds {SAMPLE_MAX_BEAM}")
    if topk > 0 and topp > 0:
        raise ValueError("sample_step: top-k and top-p exclude each other")
    dev = lprobs.device
    N = bsz * beam
    if lprobs.dtype != torch.float32 or tuple(lprobs.shape) != (N, V) or not lprobs.is_contiguous():
        raise ValueError(f"sample_step: lprobs must be contiguous fp32 [{N}, {V}], got {lprobs.dtype} "
                         f"{tuple(lprobs.shape)}")
    if ids.dtype != torch.int64 or tuple(ids.shape) != (bsz,) or ids.device != dev or not ids.is_contiguous():
        raise ValueError(f"sample_step: ids must be contiguous int64 [{bsz}] on {dev}")
    if not first_step and (prev_col is None or prev_col.dtype != torch.float32 or prev_col.numel() != N):
        raise ValueError(f"sample_step: prev_col must be an fp32 column of {N} scores after the first step")
    sc = torch.empty(bsz, beam, dtype=torch.float32, device=dev)
    lp = torch.empty(bsz, beam, dtype=torch.float32, device=dev)
    tok = torch.empty(bsz, beam, dtype=torch.int64, device=dev)
    bm = torch.empty(bsz, beam, dtype=torch.int64, device=dev)
    kept = torch.empty(bsz, beam, dtype=torch.int32, device=dev)
    ld = prev_col.stride(0) if prev_col is not None else 0
    call("mms2ut_sample_step", lprobs.data_ptr(), _p(prev_col), ld, ids.data_ptr(), bsz, beam, V, int(step),
         int(first_step), int(seed) & 0xFFFFFFFFFFFFFFFF, int(topk) if topk > 0 else 0,
         float(topp) if topp > 0 else 0.0, sc.data_ptr(), lp.data_ptr(), tok.data_ptr(), bm.data_ptr(),
         kept.data_ptr(), _s())
    return sc, tok, bm, lp, kept


def kv_cache_gather(src, dst, idx, rows):
    """dst[l, n, :rows] = src[l, idx[n], :rows] for caches [L, N, maxT, width] (idx int64 on device)."""
    L, Ns, T, W = src.shape
    Ld, N, Td, Wd = dst.shape
    if (L, T, W) != (Ld, Td, Wd) or idx.numel() != N or idx.dtype != torch.int64 or rows > T:
        raise ValueError(f"kv_cache_gather: src {tuple(src.shape)} dst {tuple(dst.shape)} idx {tuple(idx.shape)}")
    call("mms2ut_kv_cache_gather", src.data_ptr(), dst.data_ptr(), idx.data_ptr(), L, Ns, N, T, int(rows), W, _s())
    return dst


def decode_self_attn(q, cache_l, slot, N, H, hd, step_dev, kv_new, scale, out=None):
    """One decoder step of self-attention: cache_l [slots, maxT, 2*H*hd], slot int32 [>=N, maxT],
    step_dev int32 [1] (T = step + 1), kv_new [N, 2*H*hd] this step's K|V rows (stored into the cache)."""
    S, maxT, W = cache_l.shape
    if W != 2 * H * hd or slot.dtype != torch.int32 or slot.shape[1] != maxT or slot.shape[0] < N or S < N \
            or kv_new.shape[1] != W or step_dev.dtype != torch.int32:
        raise ValueError(f"decode_self_attn: cache {tuple(cache_l.shape)} slot {tuple(slot.shape)} N={N}")
    out = torch.empty(N, H * hd, dtype=F16, device=q.device) if out is None else out
    call("mms2ut_decode_self_attn", q.data_ptr(), q.stride(0), cache_l.data_ptr(), slot.data_ptr(), N, H, hd,
         maxT, step_dev.data_ptr(), kv_new.data_ptr(), kv_new.stride(0), W, out.data_ptr(), out.stride(0),
         float(scale), _s())
    return out


def decode_embed(tok, E, pos, step_dev, pad, N, D, scale, out=None):
    out = torch.empty(N, D, dtype=F16, device=E.device) if out is None else out
    call("mms2ut_decode_embed", tok.data_ptr(), E.data_ptr(), pos.data_ptr(), step_dev.data_ptr(), int(pad),
         out.data_ptr(), N, D, float(scale), _s())
    return out


def linear_splitk(x, W, bias=None, *, aux=None, relu=False, splitk=4, out=None):
    """out[M,N] = act(x @ W^T + bias) (+ aux) through `splitk` fp32 slabs and one reduction
    launch — for small-M GEMMs (the decoder step) whose dozen tiles would otherwise run long
    serial k-loops."""
    M, Kd = x.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=F16, device=x.device) if out is None else out
    slabs = torch.empty(splitk, M, N, dtype=torch.float32, device=x.device)
    gemm(x, W, slabs, M, N, Kd, lda=x.stride(0), ldb=W.stride(0), ldc=N, epi=EPI_F32, splitk=splitk,
         sCsplit=M * N)
    call("mms2ut_splitk_epilogue_f16", slabs.data_ptr(), splitk, M * N, M, N, _p(bias), _p(aux),
         aux.stride(0) if aux is not None else 0, int(relu), out.data_ptr(), out.stride(0), _s())
    return out


def linear_splitk_ln(x, W, bias, aux, g, b, eps=1e-5, *, splitk=4):
    """(xo, y): xo = x @ W^T + bias + aux (split-K slabs), y = LayerNorm(xo) — one reduction launch."""
    M, Kd = x.shape
    N = W.shape[0]
    xo = torch.empty(M, N, dtype=F16, device=x.device)
    y = torch.empty(M, N, dtype=F16, device=x.device)
    slabs = torch.empty(splitk, M, N, dtype=torch.float32, device=x.device)
    gemm(x, W, slabs, M, N, Kd, lda=x.stride(0), ldb=W.stride(0), ldc=N, epi=EPI_F32, splitk=splitk,
         sCsplit=M * N)
    call("mms2ut_splitk_epilogue_ln_f16", slabs.data_ptr(), splitk, M * N, M, N, _p(bias), aux.data_ptr(),
         aux.stride(0), xo.data_ptr(), xo.stride(0), g.data_ptr(), b.data_ptr(), float(eps), y.data_ptr(),
         y.stride(0), _s())
    return xo, y


def beam_topk(lprobs, prev_col, bsz, beam, V, k, first_step):
    """(scores [bsz,k] f32, tokens [bsz,k] i64, beams [bsz,k] i64): top-k of lprobs + prev_col per
    sentence (prev_col: a strided fp32 column view [bsz*beam] of the cumulative scores)."""
    dev = lprobs.device
    sc = torch.empty(bsz, k, dtype=torch.float32, device=dev)
    tok = torch.empty(bsz, k, dtype=torch.int64, device=dev)
    bm = torch.empty(bsz, k, dtype=torch.int64, device=dev)
    ld = prev_col.stride(0) if prev_col is not None else 0
    work = torch.empty(bsz * 32 * k, dtype=torch.int64, device=dev)
    call("mms2ut_beam_topk", lprobs.data_ptr(), _p(prev_col), ld, bsz, beam, V, int(first_step), k,
         sc.data_ptr(), tok.data_ptr(), bm.data_ptr(), work.data_ptr(), _s())
    return sc, tok, bm


def _beam_check(name, dev, *specs):
    for t, dtype, shape in specs:
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dtype} {shape} on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")


def beam_eos_scan(cand_scores, cand_indices, cands_to_ignore, eos):
    """(eos_mask [bsz,k] bool, count int32 [1] on the device): the candidates that are </s> with a
    finite score, cleared in the first `beam` columns where cands_to_ignore [bsz,beam] is set, and
    the number of true entries in those columns."""
    bsz, k = cand_scores.shape
    beam = cands_to_ignore.shape[1]
    dev = cand_scores.device
    _beam_check("beam_eos_scan", dev, (cand_scores, torch.float32, (bsz, k)), (cand_indices, torch.int64, (bsz, k)),
                (cands_to_ignore, torch.bool, (bsz, beam)))
    mask = torch.empty(bsz, k, dtype=torch.bool, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    call("mms2ut_beam_eos_scan", cand_scores.data_ptr(), cand_indices.data_ptr(), cands_to_ignore.data_ptr(), bsz,
         beam, k, int(eos), mask.data_ptr(), count.data_ptr(), _s())
    return mask, count


def beam_advance(eos_mask, cands_to_ignore, cand_scores, cand_indices, cand_beams, tokens, scores, step,
                 tokens_out, scores_out):
    """One search step's hypothesis update (mms2ut_beam_advance) -> (new cands_to_ignore [bsz,beam]
    bool, active_bbsz_idx [bsz*beam] int64); tokens_out / scores_out receive the gathered histories
    (columns [0, step+1] / [0, step]) and must not alias tokens / scores."""
    bsz, k = cand_scores.shape
    beam = cands_to_ignore.shape[1]
    dev = cand_scores.device
    N = bsz * beam
    _beam_check("beam_advance", dev, (eos_mask, torch.bool, (bsz, k)), (cands_to_ignore, torch.bool, (bsz, beam)),
                (cand_scores, torch.float32, (bsz, k)), (cand_indices, torch.int64, (bsz, k)),
                (cand_beams, torch.int64, (bsz, k)), (tokens, torch.int64, (N, tokens.shape[1])),
                (tokens_out, torch.int64, tuple(tokens.shape)), (scores, torch.float32, (N, scores.shape[1])),
                (scores_out, torch.float32, tuple(scores.shape)))
    new_ignore = torch.empty(bsz, beam, dtype=torch.bool, device=dev)
    active = torch.empty(N, dtype=torch.int64, device=dev)
    call("mms2ut_beam_advance", eos_mask.data_ptr(), cands_to_ignore.data_ptr(), cand_scores.data_ptr(),
         cand_indices.data_ptr(), cand_beams.data_ptr(), bsz, beam, k, int(step), tokens.data_ptr(),
         tokens_out.data_ptr(), tokens.shape[1], scores.data_ptr(), scores_out.data_ptr(), scores.shape[1],
         new_ignore.data_ptr(), active.data_ptr(), _s())
    return new_ignore, active


def round_up(x, m):
    return (x + m - 1) // m * m


# ============================================================================ unit vocoder

def conv1d_tm_packed_halves(Cin, Cout, taps):
    """Elements of the packed weight image of one conv1d_tm problem (vocoder.pack_conv_weight)."""
    n = ctypes.c_int64(0)
    call("mms2ut_conv1d_tm_packed_halves", int(Cin), int(Cout), int(taps), ctypes.byref(n))
    return n.value


def _rows16(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: time-major [T, C] rows expected, got {tuple(t.shape)} strides {t.stride()}")


def _f32c(t, name, n=None):
    _chk(t, torch.float32)
    if not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{name}: contiguous fp32 tensor of {n} elements expected, got {tuple(t.shape)}")


def _conv_tm_io(name, x, w_packed, t_out, Cout, taps, out, bias, res, images=1, groups=1):
    """What conv1d_tm, conv_transpose1d_tm and asr_conv check alike: x and the packed weight (`images` x
    `groups` images of Cin / groups -> Cout / groups channels and `taps` taps), out (allocated when None),
    bias and res.  t_out(T) gives the output length or raises.
    -> (T, Cin per group, T_out, out, elements of one weight image: 0 where the widths leave it undefined)."""
    _chk(x)
    _chk(w_packed)
    _rows16(x, f"{name} x")
    T, Cin_all = x.shape
    if groups < 1 or Cin_all % groups or Cout % groups:
        raise ValueError(f"{name}: {groups} groups do not divide the widths {Cin_all} -> {Cout}")
    Cin, Cog = Cin_all // groups, Cout // groups
    T_out = t_out(T)
    per = 0
    if Cin % 8 == 0 and Cin >= 8 and Cog % 8 == 0 and Cog >= 8:      # other widths: the library's message
        per = conv1d_tm_packed_halves(Cin, Cog, taps)
        if not w_packed.is_contiguous() or w_packed.numel() != images * groups * per:
            raise ValueError(f"{name}: packed weight of {w_packed.numel()} elements for {images * groups} x "
                             f"(Cin {Cin}, Cout {Cog}, taps {taps})")
    if out is None:
        out = torch.empty(T_out, Cout, dtype=F16, device=x.device)
    for t, what in ((out, "out"), (res, "res")):
        if t is not None:
            _chk(t)
            _rows16(t, f"{name} {what}")
            if tuple(t.shape) != (T_out, Cout):
                raise ValueError(f"{name}: {what} {tuple(t.shape)}, expected {(T_out, Cout)}")
    if bias is not None:
        _f32c(bias, f"{name} bias", Cout)
    return T, Cin, T_out, out, per


def conv1d_tm(x, w_packed, bias, Cout, taps, dil=1, pad=None, *, in_slope=None, res=None, out_slope=None,
              acc=_lib.VOC_ACC_NONE, scale=1.0, out=None):
    """Implicit-GEMM Conv1d over time-major fp16 rows: x [T, Cin] -> [T + 2 pad - dil (taps - 1), Cout].
    in_slope / out_slope: leaky-ReLU on the input as it is read / on the result; res: + res[t] before the
    output activation; acc SET / ADD: out = scale * v / out += scale * v (out required for ADD)."""
    pad = dil * (taps - 1) // 2 if pad is None else pad

    def t_out(T):
        if T + 2 * pad - dil * (taps - 1) < 1:
            raise ValueError(f"conv1d_tm: empty output (T {T}, taps {taps}, dilation {dil}, pad {pad})")
        return T + 2 * pad - dil * (taps - 1)

    if out is None and acc == _lib.VOC_ACC_ADD:
        raise ValueError("conv1d_tm: acc ADD needs the tensor to add into")
    T, Cin, T_out, out, _ = _conv_tm_io("conv1d_tm", x, w_packed, t_out, Cout, taps, out, bias, res)
    call("mms2ut_conv1d_tm", _lib.CONV1D_TM_ARGS.pack(
        x.data_ptr(), x.stride(0), T, Cin, w_packed.data_ptr(), 0, _p(bias) or 0, out.data_ptr(), out.stride(0),
        T_out, Cout, taps, dil, pad, T_out, 1, 1, 0, int(in_slope is not None), float(in_slope or 0.0),
        _p(res) or 0, res.stride(0) if res is not None else 0, int(acc), float(scale),
        int(out_slope is not None), float(out_slope or 0.0)), _s())
    return out


def conv_transpose1d_tm(x, w_packed, bias, Cout, k, stride, padding, *, in_slope=None, out=None):
    """ConvTranspose1d over time-major fp16 rows as `stride` polyphase convolutions in one launch:
    x [T, Cin] -> [(T - 1) stride - 2 padding + k, Cout]; w_packed from vocoder.pack_conv_transpose_weight."""
    def t_out(T):
        if (T - 1) * stride - 2 * padding + k < 1:
            raise ValueError(f"conv_transpose1d_tm: empty output (T {T}, k {k}, stride {stride}, padding {padding})")
        return (T - 1) * stride - 2 * padding + k

    T, Cin, _, out, _ = _conv_tm_io("conv_transpose1d_tm", x, w_packed, t_out, Cout, -(-k // stride), out, bias, None,
                                    images=stride)
    call("mms2ut_conv_transpose1d_tm", x.data_ptr(), x.stride(0), T, Cin, w_packed.data_ptr(), _p(bias),
         out.data_ptr(), out.stride(0), Cout, k, stride, padding, int(in_slope is not None), float(in_slope or 0.0),
         _s())
    return out


def conv_post_tanh(x, w, bias, pad, in_slope):
    """fp32 [T] = tanh(bias + Conv1d(leaky_relu(x, in_slope)) to one channel); w fp32 [taps, Cin]."""
    _chk(x)
    _chk(w, torch.float32)
    _rows16(x, "conv_post_tanh x")
    T, Cin = x.shape
    assert w.is_contiguous() and w.shape[1] == Cin
    y = torch.empty(T, dtype=torch.float32, device=x.device)
    call("mms2ut_conv_post_tanh", x.data_ptr(), x.stride(0), T, Cin, w.data_ptr(), float(bias), w.shape[0], int(pad),
         float(in_slope), y.data_ptr(), _s())
    return y


def embed_repeat(table, codes, cum=None, T_out=None):
    """fp16 [T_out, D]: row t' = table[codes[src(t')]]; cum = inclusive prefix sum of the durations
    (int64 [T], T_out = its last element) or None for src(t') = t'."""
    _chk(table)
    _chk(codes, torch.int64)
    assert table.is_contiguous() and codes.is_contiguous() and codes.dim() == 1
    T = codes.numel()
    if cum is None:
        T_out = T
    else:
        _chk(cum, torch.int64)
        assert cum.is_contiguous() and cum.numel() == T and T_out is not None
    out = torch.empty(int(T_out), table.shape[1], dtype=F16, device=table.device)
    call("mms2ut_embed_repeat", table.data_ptr(), table.shape[0], table.shape[1], codes.data_ptr(), T, _p(cum),
         int(T_out), out.data_ptr(), _s())
    return out


def var_pred_layer(x, w, b, ln_g, ln_b, *, idx=None, proj=None, eps=1e-5):
    """One fp32 VariancePredictor layer LayerNorm(ReLU(Conv1d(x))) -> fp32 [T, Cout]; w fp32
    [taps, Cin, Cout].  idx: int64 [T] row indices into x (the embedding lookup).  proj = (w [Cout],
    b): the last layer, returns (logd fp32 [T], dur int32 [T])."""
    for t in (x, w, b, ln_g, ln_b):
        _chk(t, torch.float32)
        assert t.is_contiguous()
    taps, Cin, Cout = w.shape
    assert x.shape[1] == Cin and taps % 2 == 1
    T = x.shape[0]
    if idx is not None:
        _chk(idx, torch.int64)
        assert idx.is_contiguous()
        T = idx.numel()
    out = logd = dur = pw = None
    pb = 0.0
    if proj is None:
        out = torch.empty(T, Cout, dtype=torch.float32, device=x.device)
    else:
        pw, pb = proj
        _chk(pw, torch.float32)
        assert pw.is_contiguous() and pw.numel() == Cout
        logd = torch.empty(T, dtype=torch.float32, device=x.device)
        dur = torch.empty(T, dtype=torch.int32, device=x.device)
    call("mms2ut_var_pred_layer_f32", x.data_ptr(), _p(idx), x.shape[0], T, Cin, w.data_ptr(), b.data_ptr(), taps,
         taps // 2, Cout, ln_g.data_ptr(), ln_b.data_ptr(), float(eps), _p(out), _p(pw), float(pb), _p(logd), _p(dur),
         _s())
    return out if proj is None else (logd, dur)


# ============================================================================ wav2vec2 CTC transcription

def wave_stats(x, eps=1e-7):
    """fp32 [2] = (mean, 1 / sqrt(var + eps)) of the fp32 waveform x [n] (population variance)."""
    _f32c(x, "wave_stats x")
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"wave_stats: a non-empty 1-D waveform expected, got {tuple(x.shape)}")
    ws = torch.empty(_lib.ASR_STAT_WS_DOUBLES, dtype=torch.float64, device=x.device)
    stats = torch.empty(2, dtype=torch.float32, device=x.device)
    call("mms2ut_wave_stats", x.data_ptr(), x.numel(), float(eps), ws.data_ptr(), stats.data_ptr(), _s())
    return stats


def asr_conv0(x, stats, w, bias, ln_g, ln_b, stride, eps=1e-5):
    """Feature-extractor layer 0: fp32 waveform x [n], normalised by stats (wave_stats) as it is read,
    Conv1d(1 -> C, k, stride) + LayerNorm over C + GELU -> fp16 [(n - k) // stride + 1, C]; w fp32 [k, C]."""
    _f32c(x, "asr_conv0 x")
    _f32c(stats, "asr_conv0 stats", 2)
    _chk(w, torch.float32)
    if x.dim() != 1 or w.dim() != 2 or not w.is_contiguous():
        raise ValueError("asr_conv0: x [n] and a contiguous w [k, C] expected")
    k, Cc = w.shape
    for t, nm in ((bias, "bias"), (ln_g, "ln_g"), (ln_b, "ln_b")):
        _f32c(t, "asr_conv0 " + nm, Cc)
    if x.numel() < k:
        raise ValueError(f"asr_conv0: {x.numel()} samples are fewer than the kernel's {k}")
    T0 = (x.numel() - k) // stride + 1
    y = torch.empty(T0, Cc, dtype=F16, device=x.device)
    call("mms2ut_asr_conv0", x.data_ptr(), x.numel(), stats.data_ptr(), w.data_ptr(), bias.data_ptr(), ln_g.data_ptr(),
         ln_b.data_ptr(), float(eps), int(k), int(stride), int(Cc), y.data_ptr(), y.stride(0), _s())
    return y


def asr_conv(x, w_packed, bias, Cout, taps, stride=1, pad=0, groups=1, *, T_out=None, res=None, out=None, gelu=False):
    """Strided / grouped implicit-GEMM Conv1d over time-major fp16 rows: x [T, groups * Cin] ->
    [T_out, Cout] (Cout over all groups; T_out defaults to (T + 2 pad - taps) // stride + 1).  w_packed:
    the groups' vocoder.pack_conv_weight images one after the other.  res: out = res + GELU(conv + bias).
    gelu (without res): out = GELU(conv + bias), rounded once."""
    if gelu and res is not None:
        raise ValueError("asr_conv: gelu selects the epilogue without a residual; with res the GELU is implied")

    def t_out(T):
        full = (T + 2 * pad - taps) // stride + 1
        n = full if T_out is None else int(T_out)
        if n < 1 or n > full:
            raise ValueError(f"asr_conv: {n} outputs from T {T}, taps {taps}, stride {stride}, pad {pad} (at most {full})")
        return n

    T, Cin, n_out, out, per = _conv_tm_io("asr_conv", x, w_packed, t_out, Cout, taps, out, bias, res, groups=groups)
    # a block stages input rows whose outputs belong to its neighbours: out must not overlap x (res may be x)
    x0, o0 = x.data_ptr(), out.data_ptr()
    x1, o1 = x0 + ((T - 1) * x.stride(0) + x.shape[1]) * 2, o0 + ((n_out - 1) * out.stride(0) + Cout) * 2
    if x0 < o1 and o0 < x1:
        raise ValueError("asr_conv: out overlaps x; the convolution cannot run in place")
    call("mms2ut_asr_conv", _lib.ASR_CONV_ARGS.pack(
        x.data_ptr(), x.stride(0), T, Cin, w_packed.data_ptr(), per, _p(bias) or 0, out.data_ptr(), out.stride(0),
        n_out, Cout // groups, int(taps), int(stride), int(pad), int(groups), _p(res) or 0,
        res.stride(0) if res is not None else 0, 1 if gelu else 0), _s())
    return out


def asr_ln_gelu(x, g, b, eps=1e-5):
    """x = GELU(LayerNorm(x)) in place over fp16 rows [T, C]; g, b fp32 [C]."""
    _chk(x)
    _rows16(x, "asr_ln_gelu x")
    T, Cc = x.shape
    _f32c(g, "asr_ln_gelu g", Cc)
    _f32c(b, "asr_ln_gelu b", Cc)
    if T:
        call("mms2ut_asr_ln_gelu", x.data_ptr(), x.stride(0), T, Cc, g.data_ptr(), b.data_ptr(), float(eps), _s())
    return x


def ctc_greedy(logits, V, blank, lens=None, bias=None):
    """Greedy CTC decode of fp32 logits [B, Tmax, ld >= V] (bias fp32 [V], when given, is added in place
    first) -> (ids int32 [B, Tmax] the per-frame argmax, out int32 [B, Tmax] the collapsed non-blank ids,
    count int32 [B], bad int32 [B]: 1 where an utterance has a non-finite logit).  lens int32 [B]."""
    _chk(logits, torch.float32)
    if logits.dim() != 3 or not logits.is_contiguous():
        raise ValueError(f"ctc_greedy: contiguous logits [B, Tmax, ld] expected, got {tuple(logits.shape)}")
    B, Tmax, ld = logits.shape
    if not (1 <= V <= ld) or B < 1 or Tmax < 1:
        raise ValueError(f"ctc_greedy: V {V} outside [1, {ld}] or an empty batch {tuple(logits.shape)}")
    if lens is not None:
        _chk(lens, torch.int32)
        assert lens.is_contiguous() and lens.numel() == B
    if bias is not None:
        _f32c(bias, "ctc_greedy bias", V)
    dev = logits.device
    ids = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    out = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    call("mms2ut_ctc_greedy", logits.data_ptr(), ld, int(V), B, Tmax, _p(lens), _p(bias), int(blank), ids.data_ptr(),
         out.data_ptr(), count.data_ptr(), bad.data_ptr(), _s())
    return ids, out, count, bad


# ============================================================================ speech-to-unit quantisation

def hubert_conv0(x, stats, w, bias, gn_g, gn_b, stride, eps=1e-5, *, return_stats=False):
    """HuBERT's feature-extractor layer 0: fp32 waveform x [n] (normalised by stats = wave_stats(x) as it
    is read; stats None: as it is), Conv1d(1 -> C, k, stride) (+ bias, or None), GroupNorm with one group
    per channel over all frames, GELU -> fp16 [(n - k) // stride + 1, C]; w fp32 [k, C].  return_stats:
    also the fp32 [C, 2] per-channel (mean, 1 / sqrt(var + eps)) the normalisation used."""
    _f32c(x, "hubert_conv0 x")
    if stats is not None:
        _f32c(stats, "hubert_conv0 stats", 2)
    _chk(w, torch.float32)
    if x.dim() != 1 or w.dim() != 2 or not w.is_contiguous():
        raise ValueError("hubert_conv0: x [n] and a contiguous w [k, C] expected")
    k, Cc = w.shape
    for t, nm in ((gn_g, "gn_g"), (gn_b, "gn_b")) + (((bias, "bias"),) if bias is not None else ()):
        _f32c(t, "hubert_conv0 " + nm, Cc)
    if x.numel() < k:
        raise ValueError(f"hubert_conv0: {x.numel()} samples are fewer than the kernel's {k}")
    T0 = (x.numel() - k) // stride + 1
    y = torch.empty(T0, Cc, dtype=F16, device=x.device)
    ws = torch.empty(_lib.HUBERT_GN_PARTS * Cc * 2, dtype=torch.float64, device=x.device)
    mr = torch.empty(Cc, 2, dtype=torch.float32, device=x.device)
    call("mms2ut_hubert_conv0", x.data_ptr(), x.numel(), _p(stats), w.data_ptr(), _p(bias), gn_g.data_ptr(),
         gn_b.data_ptr(), float(eps), int(k), int(stride), int(Cc), ws.data_ptr(), mr.data_ptr(), y.data_ptr(),
         y.stride(0), _s())
    return (y, mr) if return_stats else y


def kmeans_pack(centroids):
    """fp32 centroids [Kc, d] (host or device) -> (c_hi, c_lo fp16 [round_up(Kc, 16), d], cnorm fp32 [Kc]) for
    kmeans_assign, on the centroids' device: c_hi = fp16(C), c_lo = fp16((C - c_hi) * 2^11), so that
    c_hi + c_lo / 2^11 carries 22 bits of C; cnorm = |C_c|^2 summed in float64."""
    Cm = centroids.detach().to(torch.float32)
    if Cm.dim() != 2 or Cm.shape[0] < 1 or Cm.shape[1] % 8 or Cm.shape[1] < 8:
        raise ValueError(f"kmeans_pack: centroids [Kc >= 1, d a multiple of 8] expected, got {tuple(Cm.shape)}")
    if not bool(torch.isfinite(Cm).all()) or float(Cm.abs().max()) > 65504.0:
        raise ValueError("kmeans_pack: centroids must be finite and within fp16's range")
    Kc, d = Cm.shape
    hi = torch.zeros(round_up(Kc, 16), d, dtype=F16, device=Cm.device)
    lo = torch.zeros_like(hi)
    hi[:Kc] = Cm.half()
    lo[:Kc] = ((Cm - hi[:Kc].float()) * float(_lib.KMEANS_LO_SCALE)).half()
    return hi, lo, Cm.double().pow(2).sum(1).float().contiguous()


def kmeans_chunks(R, Kc, chunk=None):
    """(chunk, number of chunks) of the centroid axis for R rows: the library's choice, or a given chunk checked."""
    c, n = _lib.C.c_int(0), _lib.C.c_int(0)
    call("mms2ut_kmeans_chunks", int(R), int(Kc), int(chunk or 0), _lib.C.byref(c), _lib.C.byref(n))
    return c.value, n.value


def kmeans_assign(X, c_hi, c_lo, cnorm, lens=None, *, chunk=None):
    """Nearest centroid of every frame of fp16 X [B, Tmax, d] (or [T, d]: one utterance) against
    kmeans_pack's images: argmin_c |C_c|^2 - 2 x . C_c, the lowest index on ties, in an MFMA GEMM that
    never stores the scores.  -> (code int32 [B, Tmax], merged int32 [B, Tmax]: the codes with runs
    collapsed, count int32 [B], bad int32 [B]: 1 where a frame's best score is not finite).  lens int32
    [B]: rows past an utterance's length (anything finite) get no code.  chunk: the centroids per block
    (a multiple of 64), by default chosen so that few rows still fill the chip."""
    _chk(X)
    if X.dim() == 2:
        X = X.unsqueeze(0)
    if X.dim() != 3 or not X.is_contiguous() or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"kmeans_assign: contiguous X [B, Tmax, d] expected, got {tuple(X.shape)}")
    B, Tmax, d = X.shape
    _chk(c_hi)
    _chk(c_lo)
    Kc = cnorm.numel()
    _f32c(cnorm, "kmeans_assign cnorm")
    shape = (round_up(Kc, 16), d)
    if Kc < 1 or tuple(c_hi.shape) != shape or tuple(c_lo.shape) != shape or not c_hi.is_contiguous() \
            or not c_lo.is_contiguous():
        raise ValueError(f"kmeans_assign: centroid images {tuple(c_hi.shape)}, {tuple(c_lo.shape)}; {Kc} centroids of "
                         f"width {d} need contiguous {shape} (kmeans_pack)")
    if lens is not None:
        _chk(lens, torch.int32)
        assert lens.is_contiguous() and lens.numel() == B
    R, dev = B * Tmax, X.device
    chunk, nchunks = kmeans_chunks(R, Kc, chunk)
    pscore = torch.empty(nchunks, R, dtype=torch.float32, device=dev)
    pidx = torch.empty(nchunks, R, dtype=torch.int32, device=dev)
    code = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    merged = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    call("mms2ut_kmeans_assign", X.data_ptr(), d, R, d, c_hi.data_ptr(), c_lo.data_ptr(), cnorm.data_ptr(), Kc, chunk,
         pscore.data_ptr(), pidx.data_ptr(), _s())
    call("mms2ut_kmeans_fold", pscore.data_ptr(), pidx.data_ptr(), nchunks, B, Tmax, _p(lens), code.data_ptr(),
         merged.data_ptr(), count.data_ptr(), bad.data_ptr(), _s())
    return code, merged, count, bad


KMEANS_TOPK_MAX, UNITS_BEAM_MAX_CAND = _lib.KMEANS_TOPK_MAX, _lib.UNITS_BEAM_MAX_CAND


def check_beam_limits(top_k, beamsize=1):
    """The limits of kmeans_topk and units_beam (include/mms2ut.h), checked before anything runs."""
    top_k, beamsize = int(top_k), int(beamsize)
    if top_k < 1 or beamsize < 1:
        raise ValueError(f"top_k and beamsize must be >= 1 (got {top_k}, {beamsize})")
    if top_k > KMEANS_TOPK_MAX:
        raise NotImplementedError(f"top_k {top_k} exceeds the limit of {KMEANS_TOPK_MAX} candidates per frame")
    if beamsize * top_k > UNITS_BEAM_MAX_CAND:
        raise NotImplementedError(f"beamsize {beamsize} x top_k {top_k} exceeds the limit of {UNITS_BEAM_MAX_CAND} "
                                  "candidates per frame")
    return top_k, beamsize


def kmeans_topk(X, c_hi, c_lo, cnorm, lens=None, *, top_k=10, chunk=None):
    """The top_k nearest centroids of every frame of fp16 X [B, Tmax, d] (or [T, d]) against kmeans_pack's
    images, in kmeans_assign's GEMM with the top_k smallest (score, index) pairs per row kept on chip; no
    [rows, centroids] matrix is written.  -> (idx int32 [B, Tmax, top_k] ascending by (distance, index), so
    idx[..., 0] is kmeans_assign's code bit for bit; dist fp32 [B, Tmax, top_k] = sqrt(max(|x|^2 + score, 0)),
    the Euclidean distances; bad int32 [B]: 1 where a frame has a non-finite distance or top_k distances
    that sum to 0).  Rows past lens[b] hold zeros.  1 <= top_k <= min(32, Kc)."""
    _chk(X)
    if X.dim() == 2:
        X = X.unsqueeze(0)
    if X.dim() != 3 or not X.is_contiguous() or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"kmeans_topk: contiguous X [B, Tmax, d] expected, got {tuple(X.shape)}")
    B, Tmax, d = X.shape
    _chk(c_hi)
    _chk(c_lo)
    Kc = cnorm.numel()
    _f32c(cnorm, "kmeans_topk cnorm")
    shape = (round_up(Kc, 16), d)
    if Kc < 1 or tuple(c_hi.shape) != shape or tuple(c_lo.shape) != shape or not c_hi.is_contiguous() \
            or not c_lo.is_contiguous():
        raise ValueError(f"kmeans_topk: centroid images {tuple(c_hi.shape)}, {tuple(c_lo.shape)}; {Kc} centroids of "
                         f"width {d} need contiguous {shape} (kmeans_pack)")
    top_k, _ = check_beam_limits(top_k)
    if top_k > Kc:
        raise ValueError(f"kmeans_topk: top_k {top_k} exceeds the {Kc} centroids")
    if lens is not None:
        _chk(lens, torch.int32)
        assert lens.is_contiguous() and lens.numel() == B
    R, dev = B * Tmax, X.device
    chunk, nchunks = kmeans_chunks(R, Kc, chunk)
    pscore = torch.empty(nchunks, R, top_k, dtype=torch.float32, device=dev)
    pidx = torch.empty(nchunks, R, top_k, dtype=torch.int32, device=dev)
    idx = torch.zeros(B, Tmax, top_k, dtype=torch.int32, device=dev)
    dist = torch.zeros(B, Tmax, top_k, dtype=torch.float32, device=dev)
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    xnorm = kmeans_row_norms(X.reshape(R, d))
    call("mms2ut_kmeans_topk", X.data_ptr(), d, R, d, c_hi.data_ptr(), c_lo.data_ptr(), cnorm.data_ptr(), Kc, chunk,
         top_k, pscore.data_ptr(), pidx.data_ptr(), _s())
    call("mms2ut_kmeans_topk_fold", pscore.data_ptr(), pidx.data_ptr(), nchunks, B, Tmax, _p(lens), xnorm.data_ptr(),
         top_k, idx.data_ptr(), dist.data_ptr(), bad.data_ptr(), _s())
    return idx, dist, bad


def units_beam(idx, dist, lens=None, *, beamsize=200):
    """The reference's length-penalised beam search (mhubert.py HubertCode.decode, beamsearch=True, in
    float32) over kmeans_topk's idx int32 / dist fp32 [B, Tmax, top_k] (or [T, top_k]), one block per
    utterance of lens[b] frames; units.beam_decode_host is the host restatement it equals bit for bit.
    -> (beam_code int32 [B, Tmax], beam_merged int32 [B, Tmax]: its runs collapsed, count int32 [B], bad int32
    [B]: 1 where a frame's distances sum to 0 or to a non-finite value).  beamsize * top_k <= 2048."""
    _chk(idx, torch.int32)
    _chk(dist, torch.float32)
    if idx.dim() == 2 and dist.dim() == 2:
        idx, dist = idx.unsqueeze(0), dist.unsqueeze(0)
    if idx.dim() != 3 or idx.shape != dist.shape or not idx.is_contiguous() or not dist.is_contiguous() \
            or min(idx.shape) < 1 or dist.device != idx.device:
        raise ValueError(f"units_beam: contiguous idx, dist [B, Tmax, top_k] expected, got {tuple(idx.shape)}, "
                         f"{tuple(dist.shape)}")
    B, Tmax, top_k = idx.shape
    top_k, beamsize = check_beam_limits(top_k, beamsize)
    if lens is not None:
        _chk(lens, torch.int32)
        assert lens.is_contiguous() and lens.numel() == B
    dev = idx.device
    nbytes = _lib.i64(0)
    call("mms2ut_units_beam_ws", B, Tmax, beamsize, _lib.C.byref(nbytes))
    ws = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    code = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    merged = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    call("mms2ut_units_beam", idx.data_ptr(), dist.data_ptr(), B, Tmax, _p(lens), top_k, beamsize, ws.data_ptr(),
         code.data_ptr(), merged.data_ptr(), count.data_ptr(), bad.data_ptr(), _s())
    return code, merged, count, bad


# ============================================================================ unit codebook training (k-means)

KMEANS_PP_MAX_TRIALS = _lib.KMEANS_PP_MAX_TRIALS


def _km_rows(X, what):
    _chk(X)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 8 or X.shape[1] % 8 or not X.is_contiguous():
        raise ValueError(f"{what}: contiguous fp16 rows [N >= 1, d a multiple of 8] expected, got {tuple(X.shape)}")
    return X.shape


def kmeans_state(device):
    """The device state of a fit (include/mms2ut.h MMS_KMEANS_STATE doubles), zeroed: steps run, EWA inertia,
    its minimum, steps without improvement, done."""
    return torch.zeros(_lib.KMEANS_STATE, dtype=torch.float64, device=device)


def kmeans_row_norms(X):
    """|x|^2 of fp16 rows X [N, d] -> fp32 [N]."""
    N, d = _km_rows(X, "kmeans_row_norms")
    norms = torch.empty(N, dtype=torch.float32, device=X.device)
    call("mms2ut_kmeans_row_norms", X.data_ptr(), d, N, d, norms.data_ptr(), _s())
    return norms


def kmeans_gather(X, idx, norms=None, *, wide=False):
    """Rows idx (int32 on the device, may repeat) of fp16 X [N, d] as a contiguous batch: fp16, or fp32 with
    wide.  -> rows, or (rows, norms[idx]) given the rows' norms."""
    N, d = _km_rows(X, "kmeans_gather")
    _chk(idx, torch.int32)
    if idx.dim() != 1 or idx.numel() < 1 or not idx.is_contiguous():
        raise ValueError("kmeans_gather: a contiguous index vector expected")
    R = idx.numel()
    out = torch.empty(R, d, dtype=torch.float32 if wide else F16, device=X.device)
    nout = None
    if norms is not None:
        _f32c(norms, "kmeans_gather norms", N)
        nout = torch.empty(R, dtype=torch.float32, device=X.device)
    call("mms2ut_kmeans_gather", X.data_ptr(), d, N, _p(norms), idx.data_ptr(), R, d, out.data_ptr(), int(wide), _p(nout),
         None, _s())
    return out if norms is None else (out, nout)


def kmeans_train_assign(X, xnorm, c_hi, c_lo, cnorm, *, chunk=None):
    """The training side of kmeans_assign on fp16 rows X [R, d] with norms xnorm: -> (code int32 [R], best fp32
    [R]: the best score cnorm - 2 x . C, inertia float64 [1]: the sum of max(|x|^2 + best, 0) in double in a
    fixed order, bad int32 [1]: 1 if a best score is not finite).  No run merging, no utterances."""
    R, d = _km_rows(X, "kmeans_train_assign")
    _f32c(xnorm, "kmeans_train_assign xnorm", R)
    _chk(c_hi)
    _chk(c_lo)
    Kc = cnorm.numel()
    _f32c(cnorm, "kmeans_train_assign cnorm")
    shape = (round_up(Kc, 16), d)
    if Kc < 1 or tuple(c_hi.shape) != shape or tuple(c_lo.shape) != shape or not (c_hi.is_contiguous() and c_lo.is_contiguous()):
        raise ValueError(f"kmeans_train_assign: {Kc} centroids of width {d} need contiguous images {shape}")
    dev = X.device
    chunk, nchunks = kmeans_chunks(R, Kc, chunk)
    pscore = torch.empty(nchunks, R, dtype=torch.float32, device=dev)
    pidx = torch.empty(nchunks, R, dtype=torch.int32, device=dev)
    code = torch.empty(R, dtype=torch.int32, device=dev)
    best = torch.empty(R, dtype=torch.float32, device=dev)
    partials = torch.empty((R + 255) // 256, dtype=torch.float64, device=dev)
    inertia = torch.empty(1, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call("mms2ut_kmeans_assign", X.data_ptr(), d, R, d, c_hi.data_ptr(), c_lo.data_ptr(), cnorm.data_ptr(), Kc, chunk,
         pscore.data_ptr(), pidx.data_ptr(), _s())
    call("mms2ut_kmeans_train_fold", pscore.data_ptr(), pidx.data_ptr(), nchunks, R, xnorm.data_ptr(), code.data_ptr(),
         best.data_ptr(), partials.data_ptr(), inertia.data_ptr(), bad.data_ptr(), None, 0.0, -1, _s())
    return code, best, inertia, bad


def kmeans_accumulate(Xb, code, Kc):
    """(sums fp32 [Kc, d], cnt int32 [Kc]): per centroid the sum of the rows of fp16 Xb [R, d] whose code it is,
    added in row order in fp32, and their number.  Bitwise reproducible; no [R, Kc] array is formed."""
    R, d = _km_rows(Xb, "kmeans_accumulate")
    _chk(code, torch.int32)
    if code.numel() != R or not code.is_contiguous() or Kc < 1:
        raise ValueError(f"kmeans_accumulate: {R} codes and Kc >= 1 expected")
    sums = torch.empty(Kc, d, dtype=torch.float32, device=Xb.device)
    cnt = torch.empty(Kc, dtype=torch.int32, device=Xb.device)
    call("mms2ut_kmeans_accumulate", Xb.data_ptr(), d, code.data_ptr(), R, d, int(Kc), sums.data_ptr(), cnt.data_ptr(), None,
         _s())
    return sums, cnt


def kmeans_images(Kc, d, device):
    """Zeroed (c_hi, c_lo, cnorm) for kmeans_update to fill."""
    return (torch.zeros(round_up(Kc, 16), d, dtype=F16, device=device), torch.zeros(round_up(Kc, 16), d, dtype=F16, device=device),
            torch.zeros(Kc, dtype=torch.float32, device=device))


def kmeans_update(C, images, bad, counts=None, sums=None, cnt=None):
    """In place, one launch and no host read: where cnt > 0 the centre becomes (C * counts + sums) / (counts +
    cnt) and counts grows by cnt; then kmeans_pack's images of C into images = (c_hi, c_lo, cnorm).  Without
    counts / sums / cnt: the images only.  bad int32 [1] is set where a centre is not finite or outside
    fp16's range.  C fp32 [Kc, d], counts int64 [Kc]."""
    _chk(C, torch.float32)
    if C.dim() != 2 or not C.is_contiguous() or C.shape[1] % 8 or C.shape[1] < 8:
        raise ValueError(f"kmeans_update: contiguous centres [Kc, d a multiple of 8] expected, got {tuple(C.shape)}")
    Kc, d = C.shape
    hi, lo, cn = images
    _chk(hi)
    _chk(lo)
    _f32c(cn, "kmeans_update cnorm", Kc)
    _chk(bad, torch.int32)
    shape = (round_up(Kc, 16), d)
    if tuple(hi.shape) != shape or tuple(lo.shape) != shape or not (hi.is_contiguous() and lo.is_contiguous()):
        raise ValueError(f"kmeans_update: contiguous images {shape} expected")
    if (counts is None) != (sums is None) or (counts is None) != (cnt is None):
        raise ValueError("kmeans_update: counts, sums and cnt go together")
    if counts is not None:
        _chk(counts, torch.int64)
        _chk(cnt, torch.int32)
        _f32c(sums, "kmeans_update sums", Kc * d)
        assert counts.is_contiguous() and cnt.is_contiguous() and counts.numel() == Kc and cnt.numel() == Kc
    call("mms2ut_kmeans_update", C.data_ptr(), _p(counts), _p(sums), _p(cnt), Kc, d, hi.data_ptr(), lo.data_ptr(), cn.data_ptr(),
         bad.data_ptr(), None, _s())


def kmeans_pp(Xs, Kc, first, u):
    """k-means++ seeding over fp16 rows Xs [n, d] (csrc/kmeans.hip): row `first` is centre 0; u float64 [Kc - 1,
    trials] on the device are the uniforms of the other centres' candidates.  -> chosen int32 [Kc] (rows of
    Xs), without a host read."""
    n, d = _km_rows(Xs, "kmeans_pp")
    dev = Xs.device
    _chk(u, torch.float64)
    if u.dim() != 2 or u.shape[0] != Kc - 1 or not 1 <= u.shape[1] <= KMEANS_PP_MAX_TRIALS or not u.is_contiguous():
        raise ValueError(f"kmeans_pp: uniforms [Kc - 1, 1 .. {KMEANS_PP_MAX_TRIALS} trials] expected, got {tuple(u.shape)}")
    if not 0 <= first < n:
        raise ValueError(f"kmeans_pp: first row {first} outside [0, {n})")
    T = u.shape[1]
    closest = torch.empty(n, dtype=torch.float32, device=dev)
    dist = torch.empty(T, n, dtype=torch.float32, device=dev)
    partials = torch.empty(-(-n // _lib.KMEANS_PP_ROWS), T, dtype=torch.float64, device=dev)
    cand = torch.zeros(T, dtype=torch.int32, device=dev)
    chosen = torch.empty(Kc, dtype=torch.int32, device=dev)
    call("mms2ut_kmeans_pp", Xs.data_ptr(), n, d, int(Kc), T, int(first), u.data_ptr(), closest.data_ptr(), dist.data_ptr(),
         partials.data_ptr(), cand.data_ptr(), chosen.data_ptr(), _s())
    return chosen


class KMeansStep:
    """The buffers of a fit's mini-batch steps (mms2ut_kmeans_step_args) and the call that runs one.  X fp16 [N, d]
    with norms; C fp32 [Kc, d] (updated in place); R rows per batch.  counts, images, bad and state are made
    here: state's layout is kmeans_state's."""

    def __init__(self, X, norms, C, R, alpha, max_no_improvement):
        N, d = _km_rows(X, "KMeansStep")
        _f32c(norms, "KMeansStep norms", N)
        _chk(C, torch.float32)
        assert C.is_contiguous() and C.dim() == 2 and C.shape[1] == d
        Kc, dev = C.shape[0], X.device
        chunk, nchunks = kmeans_chunks(R, Kc)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        self.counts, self.images, self.bad, self.state = z(Kc, dt=torch.int64), kmeans_images(Kc, d, dev), \
            z(1, dt=torch.int32), kmeans_state(dev)
        self.ws = (z(R, d, dt=F16), z(R), z(nchunks, R), z(nchunks, R, dt=torch.int32), z(R, dt=torch.int32), z(R),
                   z((R + 255) // 256, dt=torch.float64), z(Kc, d), z(Kc, dt=torch.int32))
        self.keep = (X, norms, C)
        kmeans_update(C, self.images, self.bad)
        hi, lo, cn = self.images
        self.args = _lib.KMeansStepArgs(
            X.data_ptr(), d, N, norms.data_ptr(), int(R), d, Kc, chunk, C.data_ptr(), self.counts.data_ptr(), hi.data_ptr(),
            lo.data_ptr(), cn.data_ptr(), *(t.data_ptr() for t in self.ws), self.bad.data_ptr(), self.state.data_ptr(),
            float(alpha), -1 if max_no_improvement is None else int(max_no_improvement))
        self.ref = ctypes.byref(self.args)
        self.R = int(R)

    def __call__(self, idx):
        """One step on the rows idx (int32 [R] on the device); nothing is read back."""
        call("mms2ut_kmeans_step", self.ref, idx.data_ptr(), _s())


# ============================================================================ image front end (ViT features)

VISION_TILE_BYTES, VISION_MAX_SIDE = _lib.VISION_TILE_BYTES, _lib.VISION_MAX_SIDE


def vision_patches(img, desc, tab, norm, S, P, max_rows, out=None):
    """The image front end, one launch: Pillow's 8-bit bicubic resample, centre crop, normalisation and
    patchify of a batch (csrc/vision.hip).  img uint8 [bytes] and tab int32 [n] on the device; desc: the
    batch's descriptors on the host, a numpy array of the mms2ut_image_desc layout (np.dtype(_lib.ImageDesc)),
    checked here against both buffers and then uploaded; norm fp16 [3, 256].  -> fp16 [B, (S/P)^2, 3 P P]."""
    import numpy as np
    _chk(img, torch.uint8)
    _chk(tab, torch.int32)
    _chk(norm)
    dt = np.dtype(_lib.ImageDesc)
    if desc.dtype != dt or desc.ndim != 1:
        raise ValueError(f"vision_patches: desc must be a 1-d array of {dt}")
    B = desc.shape[0]
    if P < 1 or S < P or S % P:
        raise ValueError(f"vision_patches: the patch size {P} must divide the image size {S}")
    if not 1 <= max_rows <= VISION_TILE_BYTES // (3 * P):
        raise ValueError(f"vision_patches: a tile of {max_rows} source rows x {P} columns exceeds the "
                         f"{VISION_TILE_BYTES} bytes of LDS a patch may use (the image is reduced too far)")
    if tuple(norm.shape) != (3, 256) or not (norm.is_contiguous() and img.is_contiguous() and tab.is_contiguous()) \
            or img.dim() != 1 or tab.dim() != 1:
        raise ValueError("vision_patches: contiguous img [bytes], tab [n] and norm [3, 256] expected")
    nb, nt = img.numel(), tab.numel()
    for d in desc.tolist():
        src, w, h, hb, hk, hn, vb, vk, vn = d
        if not (1 <= w <= VISION_MAX_SIDE and 1 <= h <= VISION_MAX_SIDE and 0 <= src and src + 3 * w * h <= nb):
            raise ValueError(f"vision_patches: image {w}x{h} at byte {src} does not fit the buffer of {nb} bytes")
        for b, k, n in ((hb, hk, hn), (vb, vk, vn)):
            if not (n >= 1 and b >= 0 and k >= 0 and b + 2 * S <= nt and k + S * n <= nt):
                raise ValueError(f"vision_patches: table offsets ({b}, {k}, stride {n}) outside the table of {nt}")
    npatch = (S // P) ** 2
    if out is None:
        out = torch.empty(B, npatch, 3 * P * P, dtype=F16, device=img.device)
    _chk(out)
    assert out.is_contiguous() and out.numel() == B * npatch * 3 * P * P
    if B == 0:
        return out
    ddev = torch.from_numpy(desc.view(np.uint8)).to(img.device)
    call("mms2ut_vision_patches", img.data_ptr(), nb, ddev.data_ptr(), B, tab.data_ptr(), nt, norm.data_ptr(),
         out.data_ptr(), int(S), int(P), int(max_rows), _s())
    return out


def nonfinite_rows(x):
    """int32 [B]: 1 where row b of contiguous fp16 x [B, ...] holds an inf or a NaN."""
    _chk(x)
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    if not x.is_contiguous() or n % 8:
        raise ValueError(f"nonfinite_rows: contiguous rows of a multiple of 8 elements expected, got {tuple(x.shape)}")
    bad = torch.zeros(B, dtype=torch.int32, device=x.device)
    call("mms2ut_nonfinite_rows_f16", x.data_ptr(), n, B, n, bad.data_ptr(), _s())
    return bad


# ============================================================================ ViT attention rollout

ROLLOUT_MAX_T = _lib.ROLLOUT_MAX_T
ROLLOUT_FUSIONS = {"mean": 0, "max": 1, "min": 2}                   # include/mms2ut.h MMS_ROLLOUT_*
ROLLOUT_NORMALIZATIONS = {"reference": 0, "row": 1}


def rollout_discard_count(T, discard_ratio):
    """How many entries of a [T, T] matrix the discard step takes: the reference's int(T * T * ratio)."""
    if not 0.0 <= discard_ratio <= 1.0:
        raise ValueError(f"discard_ratio must be in [0, 1], got {discard_ratio}")
    return int(T * T * discard_ratio)


def rollout_probs(qkv, B, H, T, head_fusion="mean", out=None):
    """Head-fused attention probabilities of one layer from its packed fp16 qkv [B * T, 3 d] (the buffer
    mha_fwd reads: q | k | v column blocks, heads of hd = d / H columns, scale hd^-0.5) -> fp32 [B, T, T], the
    mean / max / min over heads of softmax(q k^T scale); out: a [B, T, T] view with contiguous matrices."""
    _chk(qkv)
    if head_fusion not in ROLLOUT_FUSIONS:
        raise ValueError(f"head_fusion '{head_fusion}' (one of {', '.join(ROLLOUT_FUSIONS)})")
    if T > ROLLOUT_MAX_T:
        raise NotImplementedError(f"rollout_probs: {T} tokens exceed the kernel's limit of {ROLLOUT_MAX_T}")
    if qkv.dim() != 2 or qkv.shape[0] != B * T or qkv.shape[1] % (3 * H) or qkv.stride(1) != 1 or T < 1:
        raise ValueError(f"rollout_probs: qkv [B * T, 3 d] with d a multiple of H expected, got {tuple(qkv.shape)}")
    d = qkv.shape[1] // 3
    hd = d // H
    if hd not in FLASH_HD:
        raise NotImplementedError(f"rollout_probs: head dim {hd} is not supported ({FLASH_HD})")
    if out is None:
        out = torch.empty(B, T, T, dtype=torch.float32, device=qkv.device)
    _chk(out, torch.float32)
    if tuple(out.shape) != (B, T, T) or (T > 1 and out.stride()[1:] != (T, 1)) or (B > 1 and out.stride(0) < T * T):
        raise ValueError(f"rollout_probs: out must be [B, T, T] = {(B, T, T)} with contiguous matrices")
    k = qkv[:, d:]
    call("mms2ut_rollout_probs_f16", qkv.data_ptr(), k.data_ptr(), qkv.stride(0), qkv.stride(0), B, H, T, hd,
         hd ** -0.5, ROLLOUT_FUSIONS[head_fusion], out.data_ptr(), out.stride(0) if B > 1 else T * T, _s())
    return out


def rollout_discard(x, k):
    """In place on contiguous fp32 [..., T, T] of non-negative values: per matrix the k smallest entries
    become 0 (ties at the k-th value: lower flat index first), flat index 0 is counted but kept."""
    _chk(x, torch.float32)
    if x.dim() < 2 or x.shape[-1] != x.shape[-2] or not x.is_contiguous():
        raise ValueError(f"rollout_discard: contiguous [..., T, T] expected, got {tuple(x.shape)}")
    T = x.shape[-1]
    if T > ROLLOUT_MAX_T:
        raise NotImplementedError(f"rollout_discard: {T} tokens exceed the kernel's limit of {ROLLOUT_MAX_T}")
    n = T * T
    if not 0 <= k <= n:
        raise ValueError(f"rollout_discard: k must be in [0, {n}], got {k}")
    if x.numel() and k:
        call("mms2ut_rollout_discard_f32", x.data_ptr(), x.numel() // n, n, int(k), _s())
    return x


def rollout_chain(a, normalization="reference"):
    """Processed matrices fp32 [B, L, T, T] (layers 1 .. L) -> (mask fp32 [B, T - 1], bad int32 [B]): the
    normalisation of each layer and row 0 of a_L ... a_1 over its maximum; bad[b] = 1 (and a zero mask) where
    that maximum is not positive or an entry is not finite."""
    _chk(a, torch.float32)
    if normalization not in ROLLOUT_NORMALIZATIONS:
        raise ValueError(f"normalization '{normalization}' (one of {', '.join(ROLLOUT_NORMALIZATIONS)})")
    if a.dim() != 4 or a.shape[2] != a.shape[3] or a.shape[1] < 1 or a.shape[2] < 2 or not a.is_contiguous():
        raise ValueError(f"rollout_chain: contiguous [B, L, T, T] with L >= 1, T >= 2 expected, got {tuple(a.shape)}")
    B, L, T, _ = a.shape
    if T > ROLLOUT_MAX_T:
        raise NotImplementedError(f"rollout_chain: {T} tokens exceed the kernel's limit of {ROLLOUT_MAX_T}")
    mask = torch.empty(B, T - 1, dtype=torch.float32, device=a.device)
    bad = torch.zeros(B, dtype=torch.int32, device=a.device)
    if B:
        sums = torch.empty(B, L, T, dtype=torch.float64, device=a.device)       # every matrix' row sums
        call("mms2ut_rollout_chain_f32", a.data_ptr(), B, L, T, ROLLOUT_NORMALIZATIONS[normalization], sums.data_ptr(),
             mask.data_ptr(), bad.data_ptr(), _s())
    return mask, bad


# ============================================================================ scoring (BLEU n-gram statistics, WER)

SCORE_MAX_LEN = _lib.SCORE_MAX_LEN


def _score_pairs(name, ref, ref_len, pred, pred_len):
    """The shape checks both scoring kernels share -> n_pairs.  The length limit is the library's check."""
    for t, l, what in ((ref, ref_len, "ref"), (pred, pred_len, "pred")):
        _chk(t, torch.int32)
        _chk(l, torch.int32)
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
            raise ValueError(f"{name}: {what} must be contiguous int32 [n_pairs, ld], got {tuple(t.shape)}")
        if l.dim() != 1 or l.numel() != t.shape[0] or not l.is_contiguous():
            raise ValueError(f"{name}: {what}_len must be contiguous int32 [{t.shape[0]}], got {tuple(l.shape)}")
    if ref.shape[0] != pred.shape[0]:
        raise ValueError(f"{name}: {ref.shape[0]} references against {pred.shape[0]} predictions")
    return ref.shape[0]


def ngram_stats(ref, ref_len, pred, pred_len, stats, pad, eos, unk=-1):
    """fairseq libbleu's bleu_add over a batch: right-padded int32 ref [n, ld_ref] / pred [n, ld_pred] with
    int32 lengths [n] (unk in the reference -> -999, libbleu's trims, exact n-gram matching) added into the
    device int64 stats[10] = {reflen, predlen, match1, count1, ..., match4, count4}.  Launch only: no host
    read.  Rows hold at most SCORE_MAX_LEN tokens (the library's error beyond)."""
    n = _score_pairs("ngram_stats", ref, ref_len, pred, pred_len)
    _chk(stats, torch.int64)
    if stats.numel() != 10 or not stats.is_contiguous():
        raise ValueError(f"ngram_stats: stats must be contiguous int64 [10], got {tuple(stats.shape)}")
    call("mms2ut_ngram_stats", ref.data_ptr(), ref.shape[1], ref_len.data_ptr(), pred.data_ptr(), pred.shape[1],
         pred_len.data_ptr(), n, int(pad), int(eos), -1 if unk is None else int(unk), stats.data_ptr(), _s())
    return stats


def edit_distance(ref, ref_len, pred, pred_len, totals, unk=-1, *, want_dist=False):
    """Unit-cost Levenshtein distance of every pair of a batch (layout as ngram_stats; exactly the given
    lengths, no trimming; unk in the reference -> -999), added into the device int64 totals[2] = {sum of
    distances, sum of reference lengths}.  -> int32 [n] distances with want_dist, else None.  Launch only."""
    n = _score_pairs("edit_distance", ref, ref_len, pred, pred_len)
    _chk(totals, torch.int64)
    if totals.numel() != 2 or not totals.is_contiguous():
        raise ValueError(f"edit_distance: totals must be contiguous int64 [2], got {tuple(totals.shape)}")
    dist = torch.empty(n, dtype=torch.int32, device=ref.device) if want_dist else None
    call("mms2ut_edit_distance", ref.data_ptr(), ref.shape[1], ref_len.data_ptr(), pred.data_ptr(), pred.shape[1],
         pred_len.data_ptr(), n, -1 if unk is None else int(unk), _p(dist), totals.data_ptr(), _s())
    return dist


__all__ = [n for n in dir() if not n.startswith("_")] + ["math"]
