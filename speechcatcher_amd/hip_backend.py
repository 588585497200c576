"""Backend that runs every engine op as hand-written HIP kernels through the
C ABI of libscasr.so (include/scasr.h).  torch is used only as the owner of
device memory and of the HIP stream; every pointer handed to the library is a
raw device address."""
import ctypes as C
import os
import warnings

import torch

from . import _abi


def _p(t):
    return 0 if t is None else t.data_ptr()


def resample(x, rate, device="cuda:0"):
    """A whole float32 signal (tensor or array) at ``rate`` -> a 16 kHz device tensor: sc_resample - zero history, flushed,
    the device code of the stream path - on torch's current stream.  Needs no HipBackend (the CLI converts a file with it)."""
    if not torch.cuda.is_available():
        raise _abi.ScasrError("resample needs a ROCm GPU (torch.cuda.is_available() is False)")
    lib = _abi.load()
    device = torch.device(device)
    x = torch.as_tensor(x).to(device, torch.float32).contiguous().reshape(-1)
    n_out = int(lib.sc_resample_out_count(int(rate), x.numel(), 1))
    if n_out < 0:
        _abi.check(n_out, "sc_resample_out_count")
    y = torch.empty(n_out, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        n = int(lib.sc_resample(_p(x), x.numel(), int(rate), _p(y), n_out, torch.cuda.current_stream(device).cuda_stream))
    if n != n_out:
        _abi.check(int(n) if n < 0 else -1, "sc_resample")
    return y


def segment_energy(raw_int16, device="cuda:0", smoothed=True):
    """An int16 recording at 16 kHz (numpy array or torch tensor) -> the float64 numpy array of its F curve values:
    sc_segment_energy on torch's current stream - one upload, two launches (one with ``smoothed=False``: the summed log
    filterbank energies / 10 before the Gaussian and the sign flip), one read-back.  Needs no HipBackend
    (segmenter.smoothed_negative_energy(backend="gpu") calls it)."""
    if not torch.cuda.is_available():
        raise _abi.ScasrError("segment_energy needs a ROCm GPU (torch.cuda.is_available() is False)")
    lib = _abi.load()
    device = torch.device(device)
    with warnings.catch_warnings():   # a read-only array (np.frombuffer of a WAV) is only read here
        warnings.simplefilter("ignore", UserWarning)
        x = torch.as_tensor(raw_int16)
    if x.dtype != torch.int16:
        raise TypeError(f"segment_energy takes int16 samples, got {x.dtype}")
    x = x.reshape(-1).contiguous()
    n_frames = int(lib.sc_segment_frame_count(x.numel()))
    if n_frames < 0:
        _abi.check(n_frames, "sc_segment_frame_count")
    x = x.to(device)
    out = torch.empty(n_frames, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        n = int(lib.sc_segment_energy(_p(x), x.numel(), 1 if smoothed else 0, _p(out), n_frames,
                                      torch.cuda.current_stream(device).cuda_stream))
    if n != n_frames:
        _abi.check(n if n < 0 else -1, "sc_segment_energy")
    return out.cpu().numpy()


_LEVEL_DT = [("q", "<i8", 3), ("i", "<i4", 2)]   # sc_input_level_t


def _level_dict(rec):
    from .pcm import LEVEL_FIELDS
    return dict(zip(LEVEL_FIELDS, [int(v) for v in rec["q"]] + [int(v) for v in rec["i"]]))


def decode_recording(buf, fmt, channels=1, channel=-1, scale=0, device="cuda:0", frames_per_job=1 << 16):
    """A whole recording of coded audio (bytes-like or a numpy array) -> (its float32 samples as a device tensor, its input
    level): ONE upload and ONE sc_pcm_decode launch on torch's current stream, a job per ``frames_per_job`` frames, each
    with a level of its own - all integer, so their sum on the host is the recording's level whatever the cut.  Needs no
    HipBackend (the CLI decodes a file with it)."""
    import numpy as np
    from . import pcm
    if not torch.cuda.is_available():
        raise _abi.ScasrError("decode_recording needs a ROCm GPU (torch.cuda.is_available() is False)")
    pcm.check_args(fmt, channels, channel, scale)
    lib = _abi.load()
    device = torch.device(device)
    raw = pcm.as_bytes(buf)
    bpf = pcm.bytes_per_frame(fmt, channels)
    n = raw.size // bpf
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device=device), pcm.level(b"", fmt, channels, channel, scale)
    src = torch.from_numpy(raw[:n * bpf].copy()).to(device)
    out = torch.empty(n, dtype=torch.float32, device=device)
    n_jobs = -(-n // frames_per_job)
    if n_jobs > _abi.PCM_MAX_JOBS:
        raise _abi.ScasrError(f"recording of {n} frames needs more than {_abi.PCM_MAX_JOBS} jobs of {frames_per_job}")
    levels = torch.zeros(n_jobs * 32, dtype=torch.uint8, device=device)
    tab = (_abi.PcmJob * n_jobs)()
    for k in range(n_jobs):
        j, f0 = tab[k], k * frames_per_job
        j.src, j.dst, j.level, j.level_after = src.data_ptr(), out.data_ptr() + 4 * f0, levels.data_ptr() + 32 * k, None
        j.offset, j.format, j.channels, j.channel, j.scale = f0 * bpf, fmt, channels, channel, scale
        j.n, j.restart = min(frames_per_job, n - f0), 1
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)
    with torch.cuda.device(device):
        _abi.check(lib.sc_pcm_decode(tab_dev.data_ptr(), n_jobs, torch.cuda.current_stream(device).cuda_stream), "sc_pcm_decode")
    torch.cuda.synchronize(device)
    recs = np.frombuffer(levels.cpu().numpy().tobytes(), _LEVEL_DT)
    total = pcm.zero_level()
    for r in recs:
        total = pcm.add_levels(total, _level_dict(r))
    return out, total


class DeviceLm:
    """an n-gram model on the device (sc_lm_create / sc_lm_destroy): ``view`` is the device address of its sc_lm_view,
    ``info`` a host copy of it"""

    def __init__(self, lib, blob: bytes):
        self._lib, self.handle = lib, C.c_void_p()
        buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
        rc = lib.sc_lm_create(buf, len(blob), C.byref(self.handle))
        if rc != 0:
            self.handle = None
            _abi.check(rc, "sc_lm_create")
        self.info = _abi.LmView()
        view = C.c_void_p()
        _abi.check(lib.sc_lm_device_view(self.handle, C.byref(view), C.byref(self.info)), "sc_lm_device_view")
        self.view = view.value
        self.bytes = len(blob)

    def close(self):
        if self.handle:
            self._lib.sc_lm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class DeviceGrammar:
    """a grammar on the device (sc_grammar_create / sc_grammar_destroy): ``view`` is the device address of its
    sc_grammar_view, ``info`` a host copy of it; step / accepts walk the handle's host copy"""

    def __init__(self, lib, blob: bytes):
        self._lib, self.handle = lib, C.c_void_p()
        buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
        rc = lib.sc_grammar_create(buf, len(blob), C.byref(self.handle))
        if rc != 0:
            self.handle = None
            _abi.check(rc, "sc_grammar_create")
        self.info = _abi.GrammarView()
        view = C.c_void_p()
        _abi.check(lib.sc_grammar_device_view(self.handle, C.byref(view), C.byref(self.info)), "sc_grammar_device_view")
        self.view = view.value
        self.bytes = len(blob)

    def step(self, state: int, token: int) -> int:
        return self._lib.sc_grammar_step(self.handle, int(state), int(token))

    def accepts(self, state: int) -> bool:
        return self._lib.sc_grammar_accepts(self.handle, int(state)) == 1

    def close(self):
        if self.handle:
            _abi.check(self._lib.sc_grammar_destroy(self.handle), "sc_grammar_destroy")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # (still in use: whoever holds the use lets go of it first; or the interpreter is shutting down)
            pass


class HipBackend:
    name = "hip"

    def __init__(self, device="cuda:0", use_graphs=True):
        if not torch.cuda.is_available():
            raise _abi.ScasrError("HipBackend needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _abi.load()
        self.device = torch.device(device)
        self.use_graphs = use_graphs
        self._enc_graphs = {}
        # split-K partial sums of sc_gemm live in this caller-owned workspace
        self.workspace = torch.empty(128 << 20, dtype=torch.uint8, device=self.device)
        self._chk(self.lib.sc_set_workspace(self.workspace.data_ptr(), self.workspace.numel()), "sc_set_workspace")

    def bind_stream(self, stream):
        """Give the batch that runs on `stream` its own split-K workspace, so that
        several batches can run concurrently on different HIP streams."""
        ws = torch.empty(128 << 20, dtype=torch.uint8, device=self.device)
        self._stream_ws = getattr(self, "_stream_ws", [])
        self._stream_ws.append(ws)
        self._chk(self.lib.sc_set_stream_workspace(stream.cuda_stream, ws.data_ptr(), ws.numel()),
                  "sc_set_stream_workspace")

    def check_supported(self, cfg, beam_size):
        """Reject, at construction time, model dimensions the decode kernels have no instantiation for
        (the first decode step would otherwise fail in the middle of a stream)."""
        dk = cfg.d_model // cfg.dec_heads
        if cfg.d_model % cfg.dec_heads or dk not in (16, 32, 64) or (dk == 64 and beam_size > 10):
            raise _abi.ScasrError(
                f"decoder head dim {dk} (d_model {cfg.d_model} / {cfg.dec_heads} heads) with beam {beam_size} is not "
                "supported: the HIP decoder attention kernels are instantiated for head dims 16, 32 and 64 (64: beam <= 10; "
                "csrc/search.hip)")
        ek = cfg.d_model // cfg.enc_heads
        if cfg.d_model % cfg.enc_heads or ek not in (16, 32, 64):
            raise _abi.ScasrError(f"encoder head dim {ek} is not supported (16, 32 or 64)")
        if beam_size > 16:
            raise _abi.ScasrError(f"beam size {beam_size} > 16 is not supported by the decoder attention kernels")
        if cfg.d_model % 32:
            raise _abi.ScasrError("d_model must be a multiple of 32 (sc_gemm K tiles)")
        if not 1 < cfg.vocab_size <= _abi.MAX_VOCAB:
            raise _abi.ScasrError(
                f"vocabulary size {cfg.vocab_size} is not supported (at most {_abi.MAX_VOCAB}): the full-vocabulary "
                "top-k of sc_fuse_topw keeps 8 V + 8 nextpow2(V) bytes in LDS (include/scasr.h: SC_MAX_VOCAB)")

    # ------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _chk(self, rc, what):
        if rc != 0:
            _abi.check(rc, what)

    # ------------------------------------------------------------------
    def logmel(self, w, pcm, pcap, jobs, n_jobs, max_keep, featbuf):
        cfg = w.cfg
        mode = 0 if not w.has_mvn else (2 if w.mvn_is_f64 else 1)
        self._chk(self.lib.sc_logmel(_p(pcm), pcap, _p(jobs), n_jobs, max_keep, _p(w.window), _p(w.mel_fb),
                                     _p(w.twiddle), _p(w.mean64), _p(w.std64), mode, cfg.n_fft,
                                     cfg.hop_length, cfg.win_length, cfg.n_mels, _p(featbuf),
                                     self._stream()), "sc_logmel")

    def resample(self, x, rate):
        """a whole float32 signal at ``rate`` -> 16 kHz on the device (see ``resample``)"""
        return resample(x, rate, self.device)

    def segment_energy(self, raw_int16, smoothed=True):
        """the energy curve of an int16 recording at 16 kHz as float64 numpy (see ``segment_energy``)"""
        return segment_energy(raw_int16, self.device, smoothed)

    def conv1(self, w, featbuf, jobs, n_jobs, max_t1, c1):
        cfg = w.cfg
        self._chk(self.lib.sc_conv1(_p(featbuf), cfg.n_mels, _p(jobs), n_jobs, max_t1, _p(w.conv1_w),
                                    _p(w.conv1_b), cfg.d_model, _p(c1), self._stream()), "sc_conv1")

    def gemm(self, A, a_rows, lda, W, bias, Cm, c_rows, ldc, M, N, K, relu=False, conv_f1=0,
             residual=False, naive=False, split16=False):
        flags = (1 if relu else 0) | (2 if residual else 0) | (4 if naive else 0) | (16 if split16 else 0)
        self._chk(self.lib.sc_gemm(_p(A), _p(a_rows), lda, _p(W), _p(bias), _p(Cm), _p(c_rows), ldc,
                                   M, N, K, flags, conv_f1, self._stream()), "sc_gemm")

    def gemm_ln(self, A, a_rows, lda, W, bias, Cm, c_rows, ldc, M, N, K, ln_g, ln_b, ln_out,
                relu=False, conv_f1=0, residual=False, eps=1e-12, ln_at_crows=False):
        flags = (1 if relu else 0) | (2 if residual else 0) | (8 if ln_at_crows else 0)
        self._chk(self.lib.sc_gemm_ln(_p(A), _p(a_rows), lda, _p(W), _p(bias), _p(Cm), _p(c_rows), ldc,
                                      M, N, K, flags, conv_f1, _p(ln_g), _p(ln_b), eps, _p(ln_out),
                                      ln_out.shape[-1], self._stream()), "sc_gemm_ln")

    def proj_ln_proj(self, A, lda, W1, b1, X, ldx, ln_g, ln_b, XN, W2, b2, Q, M, D, eps=1e-12, rows=None):
        self._chk(self.lib.sc_proj_ln_proj(_p(A), lda, _p(W1), _p(b1), _p(X), ldx, _p(ln_g), _p(ln_b), eps,
                                           _p(XN), D, _p(W2), _p(b2), _p(Q), D, _p(rows), M, D, self._stream()),
                  "sc_proj_ln_proj")

    def ffn_ln(self, XN, rows, M, D, F, W1p, b1, W2p, b2, X, ln_g, ln_b, ln_out, eps=1e-12):
        self._chk(self.lib.sc_ffn_ln(_p(XN), _p(rows), M, D, F, _p(W1p), _p(b1), _p(W2p), _p(b2), _p(X),
                                     _p(ln_g), _p(ln_b), eps, _p(ln_out), self._stream()), "sc_ffn_ln")

    def rowtile_proj_h(self, A, M, D, Wh, bias, N, C, ln_g=None, ln_b=None, R=None, g2=None, b2=None, LN2=None, eps=1e-12):
        """sc_rowtile_proj with fp16 weights (the packed fragments as torch.float16): fp16 MFMA inputs, fp32 accumulation"""
        assert Wh.dtype == torch.float16
        self._chk(self.lib.sc_rowtile_proj_h(_p(A), A.shape[-1], M, D, _p(ln_g), _p(ln_b), eps, _p(Wh), _p(bias), N, _p(R), _p(C),
                                             C.shape[-1], _p(g2), _p(b2), _p(LN2), self._stream()), "sc_rowtile_proj_h")

    def rowtile_proj_s(self, A, M, D, Ws, bias, N, C, ln_g=None, ln_b=None, R=None, g2=None, b2=None, LN2=None, eps=1e-12):
        """sc_rowtile_proj with the fp16 hi | lo split of the weights (weights.split_panel_weight): fp32-grade results"""
        assert Ws.dtype == torch.float16
        self._chk(self.lib.sc_rowtile_proj_s(_p(A), A.shape[-1], M, D, _p(ln_g), _p(ln_b), eps, _p(Ws), _p(bias), N, _p(R), _p(C),
                                             C.shape[-1], _p(g2), _p(b2), _p(LN2), self._stream()), "sc_rowtile_proj_s")

    def ffn_ln_h(self, XN, rows, M, D, F, W1h, b1, W2h, b2, X, ln_g, ln_b, ln_out, eps=1e-12):
        """sc_ffn_ln with fp16 weights (the packed fragments as torch.float16): fp16 MFMA inputs, fp32 accumulation"""
        assert W1h.dtype == torch.float16 and W2h.dtype == torch.float16
        self._chk(self.lib.sc_ffn_ln_h(_p(XN), _p(rows), M, D, F, _p(W1h), _p(b1), _p(W2h), _p(b2), _p(X),
                                       _p(ln_g), _p(ln_b), eps, _p(ln_out), self._stream()), "sc_ffn_ln_h")

    def ffn_ln_s(self, XN, rows, M, D, F, W1s, b1, W2s, b2, X, ln_g, ln_b, ln_out, eps=1e-12):
        """sc_ffn_ln with the fp16 hi | lo split of the weights (weights.split_panel_weight): fp32-grade results from
        fp16 MFMA inputs"""
        assert W1s.dtype == torch.float16 and W2s.dtype == torch.float16
        self._chk(self.lib.sc_ffn_ln_s(_p(XN), _p(rows), M, D, F, _p(W1s), _p(b1), _p(W2s), _p(b2), _p(X),
                                       _p(ln_g), _p(ln_b), eps, _p(ln_out), self._stream()), "sc_ffn_ln_s")

    def ffn_ln_proj(self, XN, rows, M, D, F, W1p, b1, W2p, b2, Xin, Xout, ln_g, ln_b, Wq, bq, Q, N, eps=1e-12):
        self._chk(self.lib.sc_ffn_ln_proj(_p(XN), _p(rows), M, D, F, _p(W1p), _p(b1), _p(W2p), _p(b2), _p(Xin),
                                          _p(Xout), _p(ln_g), _p(ln_b), eps, None, _p(Wq), _p(bq), _p(Q), N,
                                          self._stream()), "sc_ffn_ln_proj")

    def rowtile_proj(self, A, M, D, Wp, bias, N, C_out, ln_g=None, ln_b=None, R=None, g2=None, b2=None, LN2=None,
                     eps=1e-12):
        """C = [LN](A) . W^T + bias [+ R] [-> LN2]  (include/scasr.h: sc_rowtile_proj)"""
        self._chk(self.lib.sc_rowtile_proj(_p(A), A.shape[-1], M, D, _p(ln_g), _p(ln_b), eps, _p(Wp), _p(bias), N,
                                           _p(R), _p(C_out), C_out.shape[-1], _p(g2), _p(b2), _p(LN2),
                                           self._stream()), "sc_rowtile_proj")

    def kv_rows_to_half(self, stage, rows, m, n_layers, tcap, d2, ckv):
        self._chk(self.lib.sc_kv_rows_to_half(_p(stage), _p(rows), m, n_layers, tcap, d2, _p(ckv), self._stream()),
                  "sc_kv_rows_to_half")

    def copy_rows(self, src, src_rows, dst, dst_rows, n, width):
        self._chk(self.lib.sc_copy_rows(_p(src), _p(src_rows), _p(dst), _p(dst_rows), n, width,
                                        self._stream()), "sc_copy_rows")

    def layernorm(self, src, src_rows, dst, dst_rows, M, g, b, eps=1e-12):
        self._chk(self.lib.sc_layernorm(_p(src), _p(src_rows), src.shape[-1], _p(dst), _p(dst_rows),
                                        dst.shape[-1], M, g.numel(), _p(g), _p(b), eps,
                                        self._stream()), "sc_layernorm")

    def log_softmax_rows(self, x, rows, n, V):
        self._chk(self.lib.sc_log_softmax_rows(_p(x), _p(rows), n, V, self._stream()), "sc_log_softmax_rows")

    def block_pack(self, w, subbuf, jobs, nb, R, xblk):
        self._chk(self.lib.sc_block_pack(_p(subbuf), _p(jobs), nb, R, _p(w.pe), w.cfg.d_model, _p(xblk),
                                         self._stream()), "sc_block_pack")

    def ctx_handoff(self, x, R, jobs, ns, state, layer):
        self._chk(self.lib.sc_ctx_handoff(_p(x), R, _p(jobs), ns, _p(state), layer, x.shape[-1],
                                          self._stream()), "sc_ctx_handoff")

    def enc_attention(self, qkv, att, nblk, R, H, masked):
        self._chk(self.lib.sc_enc_attention(_p(qkv), _p(att), nblk, R, H, att.shape[-1], int(masked),
                                            self._stream()), "sc_enc_attention")

    def glu_dwconv_bn_swish(self, y, B, T, Cc, ksize, dw_w, dw_b, bn_g, bn_b, bn_mean, bn_var, eps, out):
        self._chk(self.lib.sc_glu_dwconv_bn_swish(_p(y), B, T, Cc, ksize, _p(dw_w), _p(dw_b), _p(bn_g), _p(bn_b),
                                                  _p(bn_mean), _p(bn_var), eps, _p(out), self._stream()),
                  "sc_glu_dwconv_bn_swish")

    def relpos_attention(self, qkv, p, bias_u, bias_v, out, B, T, H, mask=None):
        """mask: None, uint8 [B][T] (keys) or [B][T][T]; 0 = masked out"""
        mode = 0 if mask is None else (1 if mask.dim() == 2 else 2)
        self._chk(self.lib.sc_relpos_attention_masked(_p(qkv), _p(p), _p(bias_u), _p(bias_v), _p(out), B, T, H,
                                                      out.shape[-1], _p(mask), mode, self._stream()),
                  "sc_relpos_attention_masked")

    def _enc_layer_table(self, w):
        # cached ON the weights object (never keyed by id(): ids are recycled)
        arr = getattr(w, "_sc_enc_layer_table", None)
        if arr is None:
            arr = (_abi.EncLayer * len(w.enc))()
            for i, lw in enumerate(w.enc):
                for name, _ in _abi.EncLayer._fields_:
                    setattr(arr[i], name, lw[name].data_ptr() if name in lw else None)   # w1_h / w2_h: optional
            w._sc_enc_layer_table = arr
        return arr

    def encoder_layers(self, w, x, nblk, R, masked, jobs, ns, past_ctx, xn, qkv, att, ffh):
        """All encoder layers.  The ~360 launches are replayed from a hipGraph
        keyed by every argument that shapes the launch sequence (pointers
        included, so a cached graph is only ever replayed with the exact
        arguments it was captured with)."""
        cfg = w.cfg
        tab = self._enc_layer_table(w)
        st = self._stream()

        def launch():
            self._chk(self.lib.sc_encoder_layers(C.cast(tab, C.c_void_p), len(w.enc), _p(x), nblk, R, int(masked),
                                                 _p(jobs), ns, _p(past_ctx), _p(xn), _p(qkv), _p(att), _p(ffh),
                                                 cfg.d_model, cfg.enc_heads, cfg.ffn_dim, cfg.ln_eps,
                                                 st), "sc_encoder_layers")

        if not self.use_graphs or st == 0:
            return launch()
        key = (C.addressof(tab), _p(x), nblk, R, int(masked), _p(jobs), ns, _p(past_ctx), _p(xn), _p(qkv),
               _p(att), _p(ffh), st)
        g = self._enc_graphs.get(key)
        if g is None:
            if len(self._enc_graphs) >= 16:      # ragged callers: do not hoard graphs
                return launch()
            self._chk(self.lib.sc_graph_capture_begin(st), "sc_graph_capture_begin")
            try:
                launch()
            finally:
                out = C.c_void_p()
                rc = self.lib.sc_graph_capture_end(st, C.byref(out))
            self._chk(rc, "sc_graph_capture_end")
            self._enc_graphs[key] = g = out
        self._chk(self.lib.sc_graph_launch(g, st), "sc_graph_launch")

    def ctc_align(self, jobs):
        """Batched CTC forced alignment (sc_ctc_align), one launch pair for all jobs.  jobs: list of
        (emis [T, V] fp32 tensor, a row-major view: rows may be strided; labels int32 tensor [L]; blank).
        Returns (start [n, Lmax], end [n, Lmax], logp_mean [n, Lmax], path_score [n] fp32, status [n]) as numpy arrays;
        entries past a job's L are undefined."""
        import numpy as np
        n = len(jobs)
        Lmax = max([1] + [int(j[1].numel()) for j in jobs])
        Tmax = max([0] + [int(j[0].shape[0]) for j in jobs])
        dev = self.device
        out_i = torch.full((n, 2, Lmax), -7, dtype=torch.int32, device=dev)
        out_f = torch.zeros((n, Lmax), dtype=torch.float32, device=dev)
        ps = torch.zeros(n, dtype=torch.float32, device=dev)
        stt = torch.full((n,), -7, dtype=torch.int32, device=dev)
        ws_sizes = [(int(self.lib.sc_ctc_align_ws_bytes(int(j[0].shape[0]))) + 255) // 256 * 256 for j in jobs]
        ws = torch.empty(max(1, sum(ws_sizes)), dtype=torch.uint8, device=dev)
        tab = (_abi.AlignJob * max(1, n))()
        off = 0
        for k, (emis, labels, blank) in enumerate(jobs):
            assert emis.dtype == torch.float32 and emis.dim() == 2 and emis.stride(1) == 1
            assert labels.dtype == torch.int32 and labels.is_contiguous()
            j = tab[k]
            j.emis, j.labels, j.ws = emis.data_ptr(), labels.data_ptr() if labels.numel() else None, ws.data_ptr() + off
            j.start, j.end = out_i[k, 0].data_ptr(), out_i[k, 1].data_ptr()
            j.logp_mean, j.path_score, j.status = out_f[k].data_ptr(), ps[k].data_ptr(), stt[k].data_ptr()
            j.stride, j.T, j.L, j.V, j.blank = emis.stride(0), emis.shape[0], labels.numel(), emis.shape[1], int(blank)
            off += ws_sizes[k]
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_align(tab_dev.data_ptr(), n, Tmax, Lmax if n else 0, self._stream()), "sc_ctc_align")
        torch.cuda.synchronize(dev)
        oi = out_i.cpu().numpy()
        return oi[:, 0], oi[:, 1], out_f.cpu().numpy(), ps.cpu().numpy().astype(np.float32), stt.cpu().numpy()

    def ctc_activity(self, jobs, thr):
        """Batched CTC speech-activity scan (sc_ctc_activity), one launch for all jobs.  jobs: list of
        (table [T, V] fp32 tensor, rows may be strided; blank; t0; t1; state: six ints or None = the span starts an
        utterance).  Returns (states [n, 6] int32: the states after the spans, p_blank: list of float64 arrays [T] with the
        entries [t0, t1) written and NaN-free sentinels -7 elsewhere, states_after [n, 6]: the second copy)."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        Tmax = max([1] + [int(j[0].shape[0]) for j in jobs])
        state = torch.zeros((max(n, 1), 6), dtype=torch.int32, device=dev)
        after = torch.full((max(n, 1), 6), -7, dtype=torch.int32, device=dev)
        track = torch.full((max(n, 1), Tmax), -7.0, dtype=torch.float64, device=dev)
        tab = (_abi.ActivityJob * max(1, n))()
        for k, (table, blank, t0, t1, st) in enumerate(jobs):
            assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
            assert 0 <= t0 <= t1 <= table.shape[0]
            if st is not None:
                state[k] = torch.as_tensor(np.asarray(st, np.int32))
            j = tab[k]
            j.table, j.state, j.track, j.state_after = table.data_ptr(), state[k].data_ptr(), track[k].data_ptr(), after[k].data_ptr()
            j.stride, j.thr, j.V, j.blank, j.t0, j.t1 = table.stride(0), float(thr), table.shape[1], int(blank), int(t0), int(t1)
            j.restart = 1 if st is None else 0
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_activity(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_activity")
        torch.cuda.synchronize(dev)
        tr = track.cpu().numpy()
        return state.cpu().numpy()[:n], [tr[k, :int(jobs[k][0].shape[0])] for k in range(n)], after.cpu().numpy()[:n]

    def ctc_spot(self, jobs, labels, lens, floors, tweak=None):
        """Batched CTC phrase-spotting scan (sc_ctc_spot) on the caller's tables, one launch for all jobs.  labels
        [P, 32] int32, lens [P] int32, floors [P] float64: the phrase set (speechcatcher_amd.spotting.PhraseSet).  jobs:
        list of (table [T, V] fp32 tensor, rows may be strided; blank; t0; t1; state: a dict as returned here or None =
        the span starts an utterance; mask).  Returns (states: list of {n_frames, n_events, values [P, 64] float64,
        starts [P, 64] int32, events: the stored (end, phrase, start, score), raw_events: the events array as int32
        [64, 6]}, counters_after [n, 2] int32: the second
        copy, -7 where a job wrote nothing).  ``tweak(k, job)``: test aid, edits the sc_ctc_spot_job of job k before the
        launch; a job that starts an utterance is handed a state block filled with -7, so what it leaves unwritten shows."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        P = int(np.asarray(lens).shape[0])
        NS, NE = _abi.SPOT_STATES, _abi.SPOT_MAX_EVENTS
        lab_d = torch.as_tensor(np.ascontiguousarray(labels, np.int32).reshape(P, _abi.SPOT_MAX_LEN)).to(dev)
        len_d = torch.as_tensor(np.ascontiguousarray(lens, np.int32)).to(dev)
        flo_d = torch.as_tensor(np.ascontiguousarray(floors, np.float64)).to(dev)
        cnt = np.full((max(n, 1), 2), -7, np.int32)
        val = np.full((max(n, 1), P, NS), -7.0, np.float64)
        sta = np.full((max(n, 1), P, NS), -7, np.int32)
        evt = np.zeros((max(n, 1), NE, 6), np.int32)       # sc_spot_event: four int32 and a double
        evt[:] = -7
        for k, job in enumerate(jobs):
            st = job[4]
            if st is not None:
                cnt[k] = (st["n_frames"], st["n_events"])
                val[k], sta[k] = st["values"], st["starts"]
                for i, (end, ph, start, score) in enumerate(st["events"]):
                    evt[k, i, :4] = (end, ph, start, 0)
                    evt[k, i, 4:] = np.frombuffer(np.float64(score).tobytes(), np.int32)
        cnt_d, val_d, sta_d, evt_d = (torch.as_tensor(a).to(dev) for a in (cnt, val, sta, evt))
        after = torch.full((max(n, 1), 2), -7, dtype=torch.int32, device=dev)
        tab = (_abi.SpotJob * max(1, n))()
        for k, (table, blank, t0, t1, st, mask) in enumerate(jobs):
            assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
            assert 0 <= t0 <= t1 <= table.shape[0]
            j = tab[k]
            j.table, j.labels, j.lens, j.floors = table.data_ptr(), lab_d.data_ptr(), len_d.data_ptr(), flo_d.data_ptr()
            j.counters, j.values, j.starts = cnt_d[k].data_ptr(), val_d[k].data_ptr(), sta_d[k].data_ptr()
            j.events, j.state_after = evt_d[k].data_ptr(), after[k].data_ptr()
            j.stride, j.mask, j.V, j.blank = table.stride(0), int(mask) & ((1 << 64) - 1), table.shape[1], int(blank)
            j.t0, j.t1, j.restart, j.P = int(t0), int(t1), 1 if st is None else 0, P
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_spot(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_spot")
        torch.cuda.synchronize(dev)
        cnt, val, sta, evt = (a.cpu().numpy() for a in (cnt_d, val_d, sta_d, evt_d))
        out = []
        for k in range(n):
            ne = int(cnt[k, 1])
            ev = [(int(e[0]), int(e[1]), int(e[2]), float(np.frombuffer(e[4:].tobytes(), np.float64)[0]))
                  for e in evt[k, :max(0, min(ne, NE))]]
            out.append({"n_frames": int(cnt[k, 0]), "n_events": ne, "values": val[k], "starts": sta[k], "events": ev,
                        "raw_events": evt[k]})
        return out, after.cpu().numpy()[:n]

    def ctc_draft(self, jobs, tweak=None, guard: int = 2):
        """Batched CTC draft scan (sc_ctc_draft) on the caller's tables, one launch for all jobs.  jobs: list of (table
        [T, V] fp32 tensor, rows may be strided; blank; t0; t1; state: a dict as returned here or None = the span starts
        an utterance; capacity of the token store).  Returns (states: list of {the seven speechcatcher_amd.draft.FIELDS,
        tokens: the stored (id, start, end, conf), raw_tokens: the store and ``guard`` slots behind it as int32 [., 6]},
        states_after: the second copy, list of 7-tuples).  ``tweak(k, job)``: test aid, edits the sc_ctc_draft_job of job k
        before the launch.  A job that starts an utterance is handed a state and a store filled with -7 (the second
        copy always is), so what it leaves unwritten shows."""
        import numpy as np
        from .draft import FIELDS
        n = len(jobs)
        dev = self.device
        st_dt = np.dtype([("i", np.int32, 6), ("conf", np.float64)])
        tk_dt = np.dtype([("i", np.int32, 4), ("conf", np.float64)])
        assert st_dt.itemsize == C.sizeof(_abi.Draft) == 32 and tk_dt.itemsize == C.sizeof(_abi.DraftToken) == 24
        caps = [int(j[5]) for j in jobs]
        off = np.concatenate([[0], np.cumsum([c + guard for c in caps])]).astype(np.int64)
        state = np.zeros(max(n, 1), st_dt)
        state.view(np.int32)[:] = -7
        after = state.copy()
        store = np.zeros(max(int(off[-1]), 1), tk_dt)
        store.view(np.int32)[:] = -7
        for k, job in enumerate(jobs):
            st = job[4]
            if st is not None:
                state[k]["i"] = [st[f] for f in FIELDS[:6]]
                state[k]["conf"] = st["open_conf"]
                for i, (tid, a, b, c) in enumerate(st["tokens"]):
                    store[off[k] + i] = ((tid, a, b, 0), c)
        state_d, after_d, store_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (state, after, store))
        tab = (_abi.DraftJob * max(1, n))()
        for k, (table, blank, t0, t1, st, cap) in enumerate(jobs):
            assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
            assert 0 <= t0 <= t1 <= table.shape[0]
            j = tab[k]
            j.table, j.state, j.state_after = table.data_ptr(), state_d.data_ptr() + 32 * k, after_d.data_ptr() + 32 * k
            j.tokens = store_d.data_ptr() + 24 * int(off[k])
            j.stride, j.V, j.blank, j.t0, j.t1 = table.stride(0), table.shape[1], int(blank), int(t0), int(t1)
            j.restart, j.capacity = 1 if st is None else 0, int(cap)
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_draft(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_draft")
        torch.cuda.synchronize(dev)
        state, after = (a.cpu().numpy().view(st_dt) for a in (state_d, after_d))
        store = store_d.cpu().numpy().view(tk_dt)
        out, aft = [], []
        for k in range(n):
            d = {f: int(state[k]["i"][i]) for i, f in enumerate(FIELDS[:6])}
            d["open_conf"] = float(state[k]["conf"])
            mine = store[off[k]:off[k + 1]]
            d["tokens"] = [(int(t["i"][0]), int(t["i"][1]), int(t["i"][2]), float(t["conf"]))
                           for t in mine[:max(0, min(d["n_closed"], caps[k]))]]
            d["raw_tokens"] = mine.view(np.int32).reshape(-1, 6).copy()
            out.append(d)
            aft.append(tuple(int(v) for v in after[k]["i"]) + (float(after[k]["conf"]),))
        return out, aft

    _BEAM_ST = [("i", "<i4", 4), ("e", [("i", "<i4", 4), ("p", "<f8", 2)], 16)]   # sc_beam_t

    @classmethod
    def _beam_pack_state(cls, st, rec):
        """a state dict of ctc_beam -> rec (one element of the sc_beam_t array); "n_entries" (test aid): the stored count
        when it is not len(entries)"""
        ent = st["entries"]
        rec["i"] = (st["n_frames"], st["n_bad"], st["n_nodes"], st.get("n_entries", len(ent)))
        for r, e in enumerate(ent):
            rec["e"][r]["i"] = e[:4]
            rec["e"][r]["p"] = e[4:]

    _BEAM_LM = [("lm", "<f8", 16), ("ctx", "<i4", 16)]   # sc_beam_lm_t

    def language_model(self, blob: bytes):
        """a packed n-gram model (speechcatcher_amd.ngram.pack) validated and uploaded once (sc_lm_create)"""
        return DeviceLm(self.lib, blob)

    def ctc_beam_lm(self, jobs, model, alpha: float, beta: float, tweak=None, guard: int = 2):
        """ctc_beam through sc_ctc_beam_lm: ``model`` (language_model(), or None: the jobs run unfused) fused in with
        the weights alpha / beta.  A job's state dict may carry "side": [(lm, ctx)] beside its entries; the returned
        states do, with "raw_lm": the sc_beam_lm_t as a numpy record; the second copies are (sc_beam_t, sc_beam_lm_t)
        records.  The job handed to ``tweak`` is the sc_ctc_beam_lm_job (the plain job in its ``beam``)."""
        return self.ctc_beam(jobs, tweak, guard, fused=(model, float(alpha), float(beta)))

    _BEAM_GR = [("g", "<i4", 16)]   # sc_beam_gr_t

    def grammar(self, blob: bytes):
        """a compiled grammar (speechcatcher_amd.grammar.compile) validated and uploaded once (sc_grammar_create)"""
        return DeviceGrammar(self.lib, blob)

    def ctc_beam_grammar(self, jobs, grammars, tweak=None, guard: int = 2):
        """ctc_beam through sc_ctc_beam_grammar: ``grammars`` - one grammar() for all jobs or a list with one per job -
        choose the candidates.  A job's state dict may carry "g": the grammar's state beside each entry; the returned
        states do, with "raw_gr": the sc_beam_gr_t as a numpy record; the second copies are (sc_beam_t, sc_beam_gr_t)
        records.  The job handed to ``tweak`` is the sc_ctc_beam_gr_job (the plain job in its ``beam``)."""
        if not isinstance(grammars, (list, tuple)):
            grammars = [grammars] * len(jobs)
        assert len(grammars) == len(jobs)
        return self.ctc_beam(jobs, tweak, guard, grammars=list(grammars))

    def ctc_beam(self, jobs, tweak=None, guard: int = 2, fused=None, grammars=None):
        """Batched CTC prefix beam search (sc_ctc_beam) on the caller's tables, one launch for all jobs.  jobs: list of
        (table [T, V] fp32 tensor, rows may be strided; blank; t0; t1; state: a dict as returned here or None = the span
        starts an utterance; capacity of the node store; B; C).  Returns (states: list of {n_frames, n_bad, n_nodes,
        entries: [(node, last, len, parent, pb, pnb)] best first, nodes: the stored (parent, token, frame), raw_state: the
        sc_beam_t as a numpy record, raw_nodes: the store and ``guard`` slots behind it as int32 [., 4]}, states_after:
        the second copies as numpy records).  ``tweak(k, job)``: test aid, edits the sc_ctc_beam_job of job k before the
        launch.  A job that starts an utterance is handed a state and a store filled with -7 (the second copy always
        is), so what it leaves unwritten shows."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        st_dt = np.dtype(self._BEAM_ST)
        assert st_dt.itemsize == C.sizeof(_abi.Beam) == 528 and C.sizeof(_abi.BeamNode) == 16
        caps = [int(j[5]) for j in jobs]
        off = np.concatenate([[0], np.cumsum([c + guard for c in caps])]).astype(np.int64)
        state = np.zeros(max(n, 1), st_dt)
        state.view(np.int32)[:] = -7
        after = state.copy()
        store = np.full((max(int(off[-1]), 1), 4), -7, np.int32)
        for k, job in enumerate(jobs):
            st = job[4]
            if st is not None:
                state[k]["e"]["i"] = (-1, -1, 0, -1)
                state[k]["e"]["p"] = -np.inf
                self._beam_pack_state(st, state[k])
                for i, rec in enumerate(st["nodes"]):
                    store[off[k] + i] = tuple(rec) + (0,)
        state_d, after_d, store_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (state, after, store))
        if fused is not None:
            lm_dt = np.dtype(self._BEAM_LM)
            assert lm_dt.itemsize == C.sizeof(_abi.BeamLm) == 192
            lms = np.zeros(max(n, 1), lm_dt)
            lms.view(np.int32)[:] = -7
            lms_after = lms.copy()
            for k, job in enumerate(jobs):
                if job[4] is not None:
                    lms[k]["lm"], lms[k]["ctx"] = 0.0, 0
                    for r, (l, c) in enumerate(job[4].get("side", [])):
                        lms[k]["lm"][r], lms[k]["ctx"][r] = l, c
            lms_d, lms_after_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (lms, lms_after))
        if grammars is not None:
            assert fused is None
            gr_dt = np.dtype(self._BEAM_GR)
            assert gr_dt.itemsize == C.sizeof(_abi.BeamGr) == 64
            grs = np.zeros(max(n, 1), gr_dt)
            grs.view(np.int32)[:] = -7
            grs_after = grs.copy()
            for k, job in enumerate(jobs):
                if job[4] is not None:
                    grs[k]["g"] = 0
                    for r, g in enumerate(job[4].get("g", [])):
                        grs[k]["g"][r] = g
            grs_d, grs_after_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (grs, grs_after))
        tab = ((_abi.BeamGrJob if grammars is not None else _abi.BeamJob if fused is None else _abi.BeamLmJob) * max(1, n))()
        for k, (table, blank, t0, t1, st, cap, B, Cn) in enumerate(jobs):
            assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
            assert 0 <= t0 <= t1 <= table.shape[0]
            j = tab[k] if fused is None and grammars is None else tab[k].beam
            j.table, j.state, j.state_after = table.data_ptr(), state_d.data_ptr() + 528 * k, after_d.data_ptr() + 528 * k
            j.nodes = store_d.data_ptr() + 16 * int(off[k])
            j.stride, j.V, j.blank, j.t0, j.t1 = table.stride(0), table.shape[1], int(blank), int(t0), int(t1)
            j.restart, j.capacity, j.B, j.C = 1 if st is None else 0, int(cap), int(B), int(Cn)
            if fused is not None:
                jl = tab[k]
                jl.lm = fused[0].view if fused[0] is not None else None
                jl.lm_state, jl.lm_state_after = lms_d.data_ptr() + 192 * k, lms_after_d.data_ptr() + 192 * k
                jl.alpha, jl.beta = fused[1], fused[2]
            if grammars is not None:
                jg = tab[k]
                jg.grammar = grammars[k].view if grammars[k] is not None else None
                jg.gr_state, jg.gr_state_after = grs_d.data_ptr() + 64 * k, grs_after_d.data_ptr() + 64 * k
            if tweak is not None:
                tweak(k, tab[k])
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        if grammars is not None:
            self._chk(self.lib.sc_ctc_beam_grammar(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_beam_grammar")
        elif fused is None:
            self._chk(self.lib.sc_ctc_beam(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_beam")
        else:
            self._chk(self.lib.sc_ctc_beam_lm(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_beam_lm")
        torch.cuda.synchronize(dev)
        state, after = (a.cpu().numpy().view(st_dt) for a in (state_d, after_d))
        store = store_d.cpu().numpy().view(np.int32).reshape(-1, 4)
        out = []
        for k in range(n):
            r = state[k]
            ne = max(0, min(int(r["i"][3]), _abi.BEAM_MAX))
            d = {"n_frames": int(r["i"][0]), "n_bad": int(r["i"][1]), "n_nodes": int(r["i"][2]),
                 "entries": [tuple(int(v) for v in e["i"]) + tuple(float(v) for v in e["p"]) for e in r["e"][:ne]],
                 "raw_state": r.copy(), "raw_nodes": store[off[k]:off[k + 1]].copy()}
            d["nodes"] = [tuple(int(v) for v in rec[:3]) for rec in d["raw_nodes"][:max(0, min(d["n_nodes"], caps[k]))]]
            out.append(d)
        if fused is not None:
            lms, lms_after = (a.cpu().numpy().view(lm_dt) for a in (lms_d, lms_after_d))
            for k, d in enumerate(out):
                d["raw_lm"] = lms[k].copy()
                d["side"] = [(float(lms[k]["lm"][r]), int(lms[k]["ctx"][r])) for r in range(len(d["entries"]))]
            return out, [(after[k].copy(), lms_after[k].copy()) for k in range(n)]
        if grammars is not None:
            grs, grs_after = (a.cpu().numpy().view(gr_dt) for a in (grs_d, grs_after_d))
            for k, d in enumerate(out):
                d["raw_gr"] = grs[k].copy()
                d["g"] = [int(grs[k]["g"][r]) for r in range(len(d["entries"]))]
            return out, [(after[k].copy(), grs_after[k].copy()) for k in range(n)]
        return out, [after[k].copy() for k in range(n)]

    def ctc_beam_pack(self, jobs, tweak=None, guard: int = 2):
        """Entries of beam states as token sequences (sc_ctc_beam_pack), one launch for all jobs.  jobs: list of (state:
        a dict as returned by ctc_beam; rank; max_len; capacity of the node store, None: len(state["nodes"])).  Returns
        one dict per job: "len", "status", "node", "last", "pb", "pnb", "ids" / "frames" [min(len, max_len)], and "raw":
        (header [4 + guard], scores [2 + guard], ids / frames [max_len + guard]) - every buffer is handed over filled
        with -7, so what a job leaves unwritten shows.  ``tweak(k, job)``: test aid."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        st_dt = np.dtype(self._BEAM_ST)
        caps = [len(j[0]["nodes"]) if j[3] is None else int(j[3]) for j in jobs]
        noff = np.concatenate([[0], np.cumsum([max(c, len(j[0]["nodes"])) for c, j in zip(caps, jobs)])]).astype(np.int64)
        ooff = np.concatenate([[0], np.cumsum([int(j[2]) + guard for j in jobs])]).astype(np.int64)
        state = np.zeros(max(n, 1), st_dt)
        store = np.full((max(int(noff[-1]), 1), 4), -7, np.int32)
        for k, (st, _, _, _) in enumerate(jobs):
            state[k]["e"]["i"] = (-1, -1, 0, -1)
            state[k]["e"]["p"] = -np.inf
            self._beam_pack_state(st, state[k])
            for i, rec in enumerate(st["nodes"]):
                store[noff[k] + i] = tuple(rec) + (0,)
        state_d, store_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (state, store))
        head = torch.full((max(n, 1), 4 + guard), -7, dtype=torch.int32, device=dev)
        sc = torch.full((max(n, 1), 2 + guard), -7.0, dtype=torch.float64, device=dev)
        ids = torch.full((max(int(ooff[-1]), 1),), -7, dtype=torch.int32, device=dev)
        frames = torch.full((max(int(ooff[-1]), 1),), -7, dtype=torch.int32, device=dev)
        tab = (_abi.BeamPackJob * max(1, n))()
        for k, (st, rank, max_len, _) in enumerate(jobs):
            j = tab[k]
            j.state, j.nodes = state_d.data_ptr() + 528 * k, store_d.data_ptr() + 16 * int(noff[k])
            j.ids, j.frames = ids.data_ptr() + 4 * int(ooff[k]), frames.data_ptr() + 4 * int(ooff[k])
            j.header, j.scores = head[k].data_ptr(), sc[k].data_ptr()
            j.capacity, j.rank, j.max_len, j.reserved = caps[k], int(rank), int(max_len), 0
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_beam_pack(tab_dev.data_ptr(), n, self._stream()), "sc_ctc_beam_pack")
        torch.cuda.synchronize(dev)
        head, sc, ids, frames = (a.cpu().numpy() for a in (head, sc, ids, frames))
        out = []
        for k in range(n):
            L = max(0, min(int(head[k, 0]), int(jobs[k][2])))
            a = int(ooff[k])
            out.append({"len": int(head[k, 0]), "status": int(head[k, 1]), "node": int(head[k, 2]), "last": int(head[k, 3]),
                        "pb": float(sc[k, 0]), "pnb": float(sc[k, 1]), "ids": ids[a:a + L].tolist(),
                        "frames": frames[a:a + L].tolist(),
                        "raw": (head[k].copy(), sc[k].copy(), ids[a:int(ooff[k + 1])].copy(),
                                frames[a:int(ooff[k + 1])].copy())})
        return out

    def ctc_alternates(self, jobs, K: int, max_L=None, tweak=None, guard: int = 2):
        """Batched CTC token alternates (sc_ctc_alternates) on the caller's tables, one launch for all jobs.  jobs: list of
        (table [T, V] fp32 tensor, rows may be strided; blank; labels, start, end: int32 sequences of one length L).
        Returns (alt_ids [n, Lmax + guard, K] int32, alt_logp [n, Lmax + guard, K] float64, own_rank [n, Lmax + guard],
        status [n, Lmax + guard]): every output buffer is handed over filled with -7, so what a job leaves unwritten - the
        rows at and past its L - shows.  ``max_L``: the bound given to the launch (default: the largest L).
        ``tweak(k, job)``: test aid, edits the sc_ctc_alt_job of job k before the launch."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        Ls = [int(np.asarray(j[2]).reshape(-1).shape[0]) for j in jobs]
        Lmax = max([0] + Ls)
        rows = Lmax + guard
        ids = torch.full((max(n, 1), rows, K), -7, dtype=torch.int32, device=dev)
        logp = torch.full((max(n, 1), rows, K), -7.0, dtype=torch.float64, device=dev)
        rank = torch.full((max(n, 1), rows), -7, dtype=torch.int32, device=dev)
        stt = torch.full((max(n, 1), rows), -7, dtype=torch.int32, device=dev)
        spans = np.zeros((max(n, 1), 3, max(Lmax, 1)), np.int32)
        for k, (_, _, labels, start, end) in enumerate(jobs):
            for r, a in enumerate((labels, start, end)):
                a = np.asarray(a, np.int32).reshape(-1)
                assert a.shape[0] == Ls[k]
                spans[k, r, :Ls[k]] = a
        spans_d = torch.as_tensor(spans).to(dev)
        tab = (_abi.AltJob * max(1, n))()
        for k, (table, blank, _, _, _) in enumerate(jobs):
            assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
            j = tab[k]
            j.emis = table.data_ptr()
            j.labels, j.start, j.end = (spans_d[k, r].data_ptr() for r in range(3))
            j.alt_ids, j.alt_logp = ids[k].data_ptr(), logp[k].data_ptr()
            j.own_rank, j.status = rank[k].data_ptr(), stt[k].data_ptr()
            j.stride, j.T, j.V, j.blank, j.L = table.stride(0), table.shape[0], table.shape[1], int(blank), Ls[k]
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_ctc_alternates(tab_dev.data_ptr(), n, Lmax if max_L is None else int(max_L), int(K),
                                             self._stream()), "sc_ctc_alternates")
        torch.cuda.synchronize(dev)
        return ids.cpu().numpy()[:n], logp.cpu().numpy()[:n], rank.cpu().numpy()[:n], stt.cpu().numpy()[:n]

    def hyp_commit(self, jobs, tweak=None, guard: int = 2):
        """Committed prefix and token stability of beams (sc_hyp_commit) on the caller's device arrays, one
        launch for all jobs.  jobs: list of (yseq, xpos: int32 device tensors [n, >= L], rows may be strided; scores:
        either one float64 tensor [n, 3] of (total, decoder, ctc) triples or three float64 tensors [n]; L; from; final).
        Returns one dict per job: "L", "commit", "n_hyp", "status", "agree" [n], "tokens" / "xpos" / "stability"
        [L - from], "score", "score_dec", "score_ctc", and "raw": the job's output buffers whole (header [4 + guard],
        agree [16 + guard], ids / pos / stability [L - from + guard], totals [3 + guard]) - every buffer is handed over
        filled with -7, so what a job leaves unwritten shows.  ``tweak(k, job)``: test aid, edits the sc_hyp_commit_job of
        job k before the launch."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        tails = [max(0, int(j[3]) - int(j[4])) for j in jobs]
        ti = np.concatenate([[0], np.cumsum([t + guard for t in tails])]).astype(np.int64)
        H = _abi.COMMIT_MAX_HYPS
        head = torch.full((max(n, 1), 4 + guard), -7, dtype=torch.int32, device=dev)
        agree = torch.full((max(n, 1), H + guard), -7, dtype=torch.int32, device=dev)
        tot = torch.full((max(n, 1), 3 + guard), -7.0, dtype=torch.float64, device=dev)
        ids = torch.full((max(int(ti[-1]), 1),), -7, dtype=torch.int32, device=dev)
        pos = torch.full((max(int(ti[-1]), 1),), -7, dtype=torch.int32, device=dev)
        stab = torch.full((max(int(ti[-1]), 1),), -7.0, dtype=torch.float64, device=dev)
        tab = (_abi.CommitJob * max(1, n))()
        for k, (ys, xp, sc, L, frm, final) in enumerate(jobs):
            assert ys.dtype == xp.dtype == torch.int32 and ys.dim() == xp.dim() == 2 and ys.stride(1) == xp.stride(1) == 1
            assert ys.shape[0] == xp.shape[0] and ys.stride(0) == xp.stride(0) and L <= ys.shape[1]
            j = tab[k]
            j.yseq, j.xpos, j.row_stride = ys.data_ptr(), xp.data_ptr(), ys.stride(0)
            if isinstance(sc, (tuple, list)):
                assert all(a.dtype == torch.float64 and a.dim() == 1 and a.stride(0) == 1 for a in sc)
                j.score, j.score_dec, j.score_ctc = (a.data_ptr() for a in sc)
                j.score_stride = 1
            else:
                assert sc.dtype == torch.float64 and sc.dim() == 2 and sc.shape[1] == 3 and sc.is_contiguous()
                j.score, j.score_dec, j.score_ctc = (sc.data_ptr() + 8 * c for c in range(3))
                j.score_stride = 3
            j.header, j.agree, j.totals = head[k].data_ptr(), agree[k].data_ptr(), tot[k].data_ptr()
            j.ids, j.pos = ids.data_ptr() + 4 * int(ti[k]), pos.data_ptr() + 4 * int(ti[k])
            j.stability = stab.data_ptr() + 8 * int(ti[k])
            j.n_hyp, j.L, j.frm, j.flags = ys.shape[0], int(L), int(frm), _abi.COMMIT_FINAL if final else 0
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_hyp_commit(tab_dev.data_ptr(), n, self._stream()), "sc_hyp_commit")
        torch.cuda.synchronize(dev)
        head, agree, tot, ids, pos, stab = (a.cpu().numpy() for a in (head, agree, tot, ids, pos, stab))
        out = []
        for k in range(n):
            a, b, t = int(ti[k]), int(ti[k + 1]), tails[k]
            nh = max(0, min(int(head[k, 2]), H))
            out.append({"L": int(head[k, 0]), "commit": int(head[k, 1]), "n_hyp": int(head[k, 2]),
                        "status": int(head[k, 3]), "agree": agree[k, :nh].copy(), "tokens": ids[a:a + t].copy(),
                        "xpos": pos[a:a + t].copy(), "stability": stab[a:a + t].copy(), "score": float(tot[k, 0]),
                        "score_dec": float(tot[k, 1]), "score_ctc": float(tot[k, 2]),
                        "raw": {"header": head[k].copy(), "agree": agree[k].copy(), "ids": ids[a:b].copy(),
                                "pos": pos[a:b].copy(), "stability": stab[a:b].copy(), "totals": tot[k].copy()}})
        return out

    def lm_rescore(self, jobs, model, tweak=None, guard: int = 2):
        """N-gram rescoring of n-best lists (sc_lm_rescore) on the caller's device arrays, one launch for
        all jobs.  ``model``: language_model().  jobs: list of dicts - "rows": int32 device tensor [n, >= L], rows may be
        strided; "scores": float64 device tensor [n]; "L"; optional "lens" (a sequence of n ints; default: L each),
        "skip" (1), "strip" (-1), "state0" (-1), "lm_eos" (-1), "alpha" (0), "beta" (0), "flags" (0), "tok" (True: the
        per-label values are wanted).  Returns one dict per job: "lm", "eos_lm", "fused" (float64 [n]), "end_state",
        "order", "status" (int32 [n]), "tok_lm" ([n, width] or None) and "raw": the output buffers whole, every one
        handed over filled with -7 and ``guard`` words longer than the kernel may write.  ``tweak(k, job)``: test aid,
        edits the sc_lm_rescore_job of job k before the launch."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        H = _abi.RESCORE_MAX_HYPS
        f64 = torch.full((max(n, 1), 3, H + guard), -7.0, dtype=torch.float64, device=dev)
        i32 = torch.full((max(n, 1), 3, H + guard), -7, dtype=torch.int32, device=dev)
        widths = [max(0, int(j["L"]) - int(j.get("skip", 1))) if j.get("tok", True) else 0 for j in jobs]
        ti = np.concatenate([[0], np.cumsum([int(j["rows"].shape[0]) * w + guard for j, w in zip(jobs, widths)])])
        tok = torch.full((max(int(ti[-1]), 1),), -7.0, dtype=torch.float64, device=dev)
        keep = []
        tab = (_abi.RescoreJob * max(1, n))()
        for k, job in enumerate(jobs):
            rows, sc = job["rows"], job["scores"]
            assert rows.dtype == torch.int32 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
            assert sc.dtype == torch.float64 and sc.dim() == 1 and sc.shape[0] == rows.shape[0]
            assert int(job["L"]) <= rows.shape[1]
            j = tab[k]
            j.model = model.view
            j.yseq, j.row_stride = rows.data_ptr(), rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], 1)
            j.score, j.score_stride = sc.data_ptr(), sc.stride(0) if sc.shape[0] > 1 else 1
            if job.get("lens") is not None:
                lens = torch.tensor([int(v) for v in job["lens"]], dtype=torch.int32, device=dev)
                keep.append(lens)
                j.lens = lens.data_ptr()
            j.fused, j.lm, j.eos_lm = (f64[k, c].data_ptr() for c in range(3))
            j.end_state, j.order, j.status = (i32[k, c].data_ptr() for c in range(3))
            if job.get("tok", True):
                j.tok_lm, j.tok_stride = tok.data_ptr() + 8 * int(ti[k]), widths[k]
            j.alpha, j.beta = float(job.get("alpha", 0.0)), float(job.get("beta", 0.0))
            j.n_hyp, j.L, j.skip, j.strip = rows.shape[0], int(job["L"]), int(job.get("skip", 1)), int(job.get("strip", -1))
            j.state0, j.lm_eos, j.V, j.flags = (int(job.get("state0", -1)), int(job.get("lm_eos", -1)), model.info.V,
                                                int(job.get("flags", 0)))
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_lm_rescore(tab_dev.data_ptr(), n, self._stream()), "sc_lm_rescore")
        torch.cuda.synchronize(dev)
        f64, i32, tok = f64.cpu().numpy(), i32.cpu().numpy(), tok.cpu().numpy()
        out = []
        for k, job in enumerate(jobs):
            nh, w = int(job["rows"].shape[0]), widths[k]
            a, b = int(ti[k]), int(ti[k + 1])
            out.append({"fused": f64[k, 0, :nh].copy(), "lm": f64[k, 1, :nh].copy(), "eos_lm": f64[k, 2, :nh].copy(),
                        "end_state": i32[k, 0, :nh].copy(), "order": i32[k, 1, :nh].copy(),
                        "status": i32[k, 2, :nh].copy(),
                        "tok_lm": tok[a:a + nh * w].reshape(nh, w).copy() if job.get("tok", True) else None,
                        "raw": {"f64": f64[k].copy(), "i32": i32[k].copy(), "tok": tok[a:b].copy()}})
        return out

    # ---- consensus of n-best lists (csrc/mbr.hip) ---------------------------------------------------------
    def mbr(self, jobs, tweak=None, guard: int = 2, ws_limit=None, ws_bytes=None):
        """Minimum-Bayes-risk row and slot confidences of n-best lists (sc_mbr) on the caller's device
        arrays.  jobs: list of dicts - "rows": int32 device tensor [n, >= L], rows may be strided; "weights" OR "scores":
        float64 device tensor [n] (scores may be strided); "L"; "V"; optional "lens" (n ints; default: L each), "skip"
        (0), "strip" (-1), "scale" (1.0), "pivot" (-1), "slots" (True: wanted).  ``ws_limit``: bytes of workspace a call
        may use - beyond it the jobs go in slabs of whole lists, one sc_mbr call each; ``ws_bytes``: the size handed to
        the one call instead of what sc_mbr_ws_bytes asks for (test aid).  Returns one dict per job: "weight", "risk"
        (float64 [n]), "dist" (int32 [16, 16]), "order", "status" (int32 [n]), "header" (int32 [4]), "conf", "alt_mass"
        (float64 [m_P]), "alt_tok" (int32 [m_P]), "gap_mass" (float64 [m_P + 1] or empty), "slots" (int32 [n, m_P] or
        None) and "raw": the output buffers whole, every one handed over filled with -7 and ``guard`` words longer than
        the kernel may write.  ``tweak(k, job)``: test aid, edits the sc_mbr_job of job k before the launch."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        H = _abi.MBR_MAX_HYPS
        caps = [min(max(0, int(j["L"]) - int(j.get("skip", 0))), _abi.MBR_MAX_LEN) for j in jobs]
        f64 = torch.full((max(n, 1), 2, H + guard), -7.0, dtype=torch.float64, device=dev)
        i32 = torch.full((max(n, 1), 2, H + guard), -7, dtype=torch.int32, device=dev)
        dist = torch.full((max(n, 1), H * H + guard), -7, dtype=torch.int32, device=dev)
        head = torch.full((max(n, 1), 4 + guard), -7, dtype=torch.int32, device=dev)
        pi = np.concatenate([[0], np.cumsum([c + 1 + guard for c in caps])]).astype(np.int64)
        pos = torch.full((3, max(int(pi[-1]), 1)), -7.0, dtype=torch.float64, device=dev)     # conf, alt_mass, gap_mass
        atok = torch.full((max(int(pi[-1]), 1),), -7, dtype=torch.int32, device=dev)
        si = np.concatenate([[0], np.cumsum([int(j["rows"].shape[0]) * c + guard if j.get("slots", True) else 0
                                             for j, c in zip(jobs, caps)])]).astype(np.int64)
        slots = torch.full((max(int(si[-1]), 1),), -7, dtype=torch.int32, device=dev)
        keep = []
        tab = (_abi.MbrJob * max(1, n))()
        for k, job in enumerate(jobs):
            rows = job["rows"]
            assert rows.dtype == torch.int32 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
            assert int(job["L"]) <= rows.shape[1] and ("weights" in job) != ("scores" in job)
            j = tab[k]
            j.yseq, j.row_stride = rows.data_ptr(), rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], 1)
            v = job["weights"] if "weights" in job else job["scores"]
            assert v.dtype == torch.float64 and v.dim() == 1 and v.shape[0] == rows.shape[0]
            if "weights" in job:
                assert v.shape[0] <= 1 or v.stride(0) == 1
                j.weight = v.data_ptr()
            else:
                j.score, j.score_stride = v.data_ptr(), v.stride(0) if v.shape[0] > 1 else 1
            if job.get("lens") is not None:
                lens = torch.tensor([int(x) for x in job["lens"]], dtype=torch.int32, device=dev)
                keep.append(lens)
                j.lens = lens.data_ptr()
            j.weight_out, j.risk = f64[k, 0].data_ptr(), f64[k, 1].data_ptr()
            j.order, j.status = i32[k, 0].data_ptr(), i32[k, 1].data_ptr()
            j.dist, j.header = dist[k].data_ptr(), head[k].data_ptr()
            j.conf, j.alt_mass, j.gap_mass = (pos[c].data_ptr() + 8 * int(pi[k]) for c in range(3))
            j.alt_tok = atok.data_ptr() + 4 * int(pi[k])
            if job.get("slots", True):
                j.slots, j.slot_stride = slots.data_ptr() + 4 * int(si[k]), caps[k]
            j.scale = float(job.get("scale", 1.0))
            j.n_hyp, j.L, j.skip, j.strip = rows.shape[0], int(job["L"]), int(job.get("skip", 0)), int(job.get("strip", -1))
            j.V, j.pivot, j.flags, j.reserved = int(job["V"]), int(job.get("pivot", -1)), 0, 0
            if tweak is not None:
                tweak(k, j)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        need = lambda a, b: int(self.lib.sc_mbr_ws_bytes(b - a, max(caps[a:b], default=0)))   # noqa: E731
        slabs, a = [], 0
        while a < n:
            b = a + 1
            while ws_limit is not None and b < n and need(a, b + 1) <= ws_limit:
                b += 1
            if ws_limit is None:
                b = n
            slabs.append((a, b))
            a = b
        self.mbr_slabs = len(slabs)
        ws_size = max([need(a, b) for a, b in slabs] + [int(ws_bytes or 0), 256])
        ws = torch.empty((ws_size,), dtype=torch.uint8, device=dev)
        for a, b in slabs:
            size = need(a, b) if ws_bytes is None else int(ws_bytes)
            self._chk(self.lib.sc_mbr(tab_dev.data_ptr() + a * C.sizeof(_abi.MbrJob), b - a, ws.data_ptr(), size,
                                      self._stream()), "sc_mbr")
        torch.cuda.synchronize(dev)
        f64, i32, dist, head, pos, atok, slots = (t.cpu().numpy() for t in (f64, i32, dist, head, pos, atok, slots))
        out = []
        for k, job in enumerate(jobs):
            nh, c = int(job["rows"].shape[0]), caps[k]
            mp = max(0, min(int(head[k, 1]), c))
            a, b = int(pi[k]), int(pi[k + 1])
            sa, sb = int(si[k]), int(si[k + 1])
            has_pivot = int(head[k, 0]) >= 0
            want_slots = bool(job.get("slots", True))
            out.append({"weight": f64[k, 0, :nh].copy(), "risk": f64[k, 1, :nh].copy(),
                        "dist": dist[k, :H * H].reshape(H, H).copy(), "order": i32[k, 0, :nh].copy(),
                        "status": i32[k, 1, :nh].copy(), "header": head[k, :4].copy(),
                        "conf": pos[0, a:a + mp].copy(), "alt_mass": pos[1, a:a + mp].copy(),
                        "gap_mass": pos[2, a:a + mp + 1].copy() if has_pivot else np.zeros(0, np.float64),
                        "alt_tok": atok[a:a + mp].copy(),
                        "slots": (slots[sa:sa + nh * c].reshape(nh, c)[:, :mp].copy() if want_slots else None),
                        "raw": {"f64": f64[k].copy(), "i32": i32[k].copy(), "dist": dist[k].copy(), "header": head[k].copy(),
                                "pos": pos[:3, a:b].copy(), "alt_tok": atok[a:b].copy(), "slots": slots[sa:sb].copy()}})
        return out

    # ---- attention rescoring of n-best lists (csrc/dec_rescore.hip) -------------------------------------
    def seq_attention(self, jobs, dk: int, max_Lq=None, tweak=None):
        """Attention of whole sequences (sc_seq_attention), one call for all jobs.  jobs: list of dicts - "q" [>= Lq,
        >= H * dk], "k", "v" [>= Lk, >= H * dk] and "o" [>= Lq, >= H * dk]: float32 device tensors whose rows may be
        strided, "Lq", "Lk", "H", "causal".  The outputs are written into the jobs' "o".  ``tweak(k, job)``: test aid,
        edits the sc_seq_attn_job of job k before the launch."""
        n = len(jobs)
        tab = (_abi.SeqAttnJob * max(1, n))()
        forms = 0
        for k, job in enumerate(jobs):
            j = tab[k]
            for name in ("q", "k", "v", "o"):
                t = job[name]
                assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
                setattr(j, name, t.data_ptr())
                setattr(j, name + "_stride", t.stride(0))
            j.Lq, j.Lk, j.H, j.causal = int(job["Lq"]), int(job["Lk"]), int(job["H"]), int(bool(job["causal"]))
            assert j.Lq <= job["q"].shape[0] and j.Lq <= job["o"].shape[0] and j.Lk <= min(job["k"].shape[0], job["v"].shape[0])
            assert j.H * dk <= min(job[name].shape[1] for name in ("q", "k", "v", "o"))
            forms |= 2 if j.causal else 1
            if tweak is not None:
                tweak(k, j)
        max_Lq = max([int(j["Lq"]) for j in jobs], default=0) if max_Lq is None else max_Lq
        max_H = max([int(j["H"]) for j in jobs], default=1)
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
        self._chk(self.lib.sc_seq_attention(tab_dev.data_ptr(), n, dk, max_Lq, max_H, forms or 1, self._stream()),
                  "sc_seq_attention")
        torch.cuda.synchronize(self.device)

    def decoder_model(self, w, LCAP: int):
        """The model part of an sc_search for sc_dec_rescore from PackedWeights ``w``: dims, ids and the fp32 decoder
        weights; no search buffers.  Returns an object that keeps everything alive: .struct (the _abi.Search), .wkv /
        .bkv (the layers' cross-attention K|V weights and biases one behind the other), .pe_rows."""
        cfg = w.cfg
        layers = (_abi.DecLayer * len(w.dec))()
        for i, lw in enumerate(w.dec):
            for name, _ in _abi.DecLayer._fields_:
                if name in lw and lw[name].dtype == torch.float32:
                    setattr(layers[i], name, lw[name].data_ptr())
        s = _abi.Search()
        s.V, s.d, s.H, s.F, s.n_layers, s.LCAP = cfg.vocab_size, cfg.d_model, cfg.dec_heads, cfg.ffn_dim, cfg.dec_layers, LCAP
        s.blank, s.eos, s.sos, s.ln_eps = cfg.blank_id, cfg.eos_id, cfg.sos_id, cfg.ln_eps
        s.embed, s.pe = w.embed.data_ptr(), w.pe.data_ptr()
        s.dec_norm_g, s.dec_norm_b = w.dec_norm_g.data_ptr(), w.dec_norm_b.data_ptr()
        s.out_w, s.out_b = w.out_w.data_ptr(), w.out_b.data_ptr()
        s.layers = C.cast(layers, C.c_void_p).value

        class _Model:
            pass
        m = _Model()
        m.struct, m.layers, m.w, m.pe_rows = s, layers, w, int(w.pe.shape[0])
        m.wkv = torch.cat([lw["wkv"] for lw in w.dec], 0).contiguous()
        m.bkv = torch.cat([lw["bkv"] for lw in w.dec], 0).contiguous()
        return m

    def dec_rescore(self, jobs, model, ws_bytes=None, tweak=None, guard: int = 2):
        """Attention rescoring of n-best lists (sc_dec_rescore) on the caller's device arrays.  ``model``:
        decoder_model().  jobs: list of dicts - "E": float32 device tensor [T, >= d] (rows may be strided) or None;
        "rows": int32 device tensor [n, >= L]; "scores": float64 device tensor [n]; "L"; optional "lens" (n ints; default
        L each), "w_att" (1), "w_ctc" (0.5), "beta" (0), "tok" (True), "pe_rows" (the model's).  ``ws_bytes``: size of the
        workspace handed over (default: what all jobs need at once) - a smaller one makes the call run in slabs.
        Returns one dict per job: "att", "fused" (float64 [n]), "order", "status" (int32 [n]), "tok_att" ([n, L + 1] or
        None) and "raw": the output buffers whole, every one handed over filled with -7 and ``guard`` words longer than
        the kernel may write.  ``tweak(k, job)``: test aid, edits the sc_dec_rescore_job of job k before the call."""
        import numpy as np
        n = len(jobs)
        dev = self.device
        H = _abi.ATT_MAX_HYPS
        f64 = torch.full((max(n, 1), 2, H + guard), -7.0, dtype=torch.float64, device=dev)
        i32 = torch.full((max(n, 1), 2, H + guard), -7, dtype=torch.int32, device=dev)
        widths = [int(j["L"]) + 1 if j.get("tok", True) else 0 for j in jobs]
        ti = np.concatenate([[0], np.cumsum([int(j["rows"].shape[0]) * w + guard for j, w in zip(jobs, widths)])])
        tok = torch.full((max(int(ti[-1]), 1),), -7.0, dtype=torch.float64, device=dev)
        keep = []
        tab = (_abi.DecRescoreJob * max(1, n))()
        rows_total = enc_total = seqs = 0
        for k, job in enumerate(jobs):
            rows, sc, E = job["rows"], job["scores"], job.get("E")
            assert rows.dtype == torch.int32 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
            assert sc.dtype == torch.float64 and sc.dim() == 1 and sc.shape[0] == rows.shape[0]
            assert int(job["L"]) <= rows.shape[1]
            j = tab[k]
            if E is not None and E.shape[0] > 0:
                assert E.dtype == torch.float32 and E.dim() == 2 and E.stride(1) == 1 and E.shape[1] >= model.struct.d
                j.E, j.e_stride, j.T = E.data_ptr(), E.stride(0), E.shape[0]
            j.yseq, j.row_stride = rows.data_ptr(), rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], 1)
            j.score, j.score_stride = sc.data_ptr(), sc.stride(0) if sc.shape[0] > 1 else 1
            if job.get("lens") is not None:
                lens = torch.tensor([int(v) for v in job["lens"]], dtype=torch.int32, device=dev)
                keep.append(lens)
                j.lens = lens.data_ptr()
            j.wkv, j.bkv = model.wkv.data_ptr(), model.bkv.data_ptr()
            j.att, j.fused = (f64[k, c].data_ptr() for c in range(2))
            j.order, j.status = (i32[k, c].data_ptr() for c in range(2))
            if job.get("tok", True):
                j.tok_att, j.tok_stride = tok.data_ptr() + 8 * int(ti[k]), widths[k]
            j.w_att, j.w_ctc, j.beta = float(job.get("w_att", 1.0)), float(job.get("w_ctc", 0.5)), float(job.get("beta", 0.0))
            j.n_hyp, j.L, j.pe_rows = rows.shape[0], int(job["L"]), int(job.get("pe_rows", model.pe_rows))
            if tweak is not None:
                tweak(k, j)
            rows_total += max(0, j.n_hyp) * (max(0, j.L) + 1)
            enc_total += max(0, j.T)
            seqs += max(0, j.n_hyp)
        need = int(self.lib.sc_dec_rescore_ws_bytes(C.addressof(model.struct), rows_total, enc_total, seqs, n))
        # (the two-GEMM feed-forward of a stream without split-K workspace keeps its hidden rows too)
        need += rows_total * model.struct.F * 4 + 256
        ws = torch.empty(max(256, need if ws_bytes is None else int(ws_bytes)), dtype=torch.uint8, device=dev)
        self._chk(self.lib.sc_dec_rescore(C.cast(tab, C.c_void_p), n, C.addressof(model.struct), ws.data_ptr(), ws.numel(),
                                          self._stream()), "sc_dec_rescore")
        torch.cuda.synchronize(dev)
        f64, i32, tok = f64.cpu().numpy(), i32.cpu().numpy(), tok.cpu().numpy()
        out = []
        for k, job in enumerate(jobs):
            nh, w = int(job["rows"].shape[0]), widths[k]
            a, b = int(ti[k]), int(ti[k + 1])
            out.append({"att": f64[k, 0, :nh].copy(), "fused": f64[k, 1, :nh].copy(),
                        "order": i32[k, 0, :nh].copy(), "status": i32[k, 1, :nh].copy(),
                        "tok_att": tok[a:a + nh * w].reshape(nh, w).copy() if job.get("tok", True) else None,
                        "raw": {"f64": f64[k].copy(), "i32": i32[k].copy(), "tok": tok[a:b].copy()}})
        return out

    def decode_pcm(self, jobs, tweak=None, guard: int = 4):
        """Batched decode of coded audio (sc_pcm_decode) on the caller's buffers, one launch for all jobs.  jobs: list of
        (src: a bytes-like object, a numpy array or a uint8 device tensor; byte offset; format; channels; channel; scale;
        n frames; level: a dict as returned here or None = the chunk starts an utterance).  Returns (samples: list of
        float32 arrays [n + guard] whose last ``guard`` entries were handed over as NaN with payload 0x7fc0dead - what a
        job leaves unwritten shows -, levels: list of dicts (the five speechcatcher_amd.pcm.LEVEL_FIELDS), levels_after:
        the second copy).  ``tweak(k, job)``: test aid, edits the sc_pcm_job of job k before the launch.  A job that
        starts an utterance is handed a level filled with -7 (the second copy always is)."""
        import numpy as np
        from . import pcm
        n = len(jobs)
        dev = self.device
        assert np.dtype(_LEVEL_DT).itemsize == C.sizeof(_abi.InputLevel) == 32
        lv = np.zeros(max(n, 1), _LEVEL_DT)
        lv.view(np.int32)[:] = -7
        after = lv.copy()
        srcs, outs = [], []
        for k, (src, offset, fmt, channels, channel, scale, nf, level) in enumerate(jobs):
            if level is not None:
                lv[k]["q"] = [level[f] for f in pcm.LEVEL_FIELDS[:3]]
                lv[k]["i"] = [level[f] for f in pcm.LEVEL_FIELDS[3:]]
            if not isinstance(src, torch.Tensor):
                src = torch.from_numpy(pcm.as_bytes(src).copy())
            assert src.dtype == torch.uint8 and src.dim() == 1
            srcs.append(src.to(dev) if src.numel() else torch.zeros(1, dtype=torch.uint8, device=dev))
            o = torch.full((max(0, int(nf)) + guard,), 0x7fc0dead, dtype=torch.int32, device=dev)
            outs.append(o)
        lv_d, after_d = (torch.as_tensor(a.view(np.uint8).copy()).to(dev) for a in (lv, after))
        tab = (_abi.PcmJob * max(1, n))()
        for k, (src, offset, fmt, channels, channel, scale, nf, level) in enumerate(jobs):
            j = tab[k]
            j.src, j.dst, j.level, j.level_after = srcs[k].data_ptr(), outs[k].data_ptr(), lv_d.data_ptr() + 32 * k, after_d.data_ptr() + 32 * k
            j.offset, j.format, j.channels, j.channel, j.scale = int(offset), int(fmt), int(channels), int(channel), int(scale)
            j.n, j.restart = int(nf), 1 if level is None else 0
            if tweak is not None:
                tweak(k, j)
            # the bounds of a well-formed job are checked HERE: the kernel trusts offset and n
            if (j.src == srcs[k].data_ptr() and 0 <= j.format < pcm.N_FORMATS and 1 <= j.channels <= pcm.MAX_CHANNELS
                    and j.n >= 0 and j.offset >= 0):
                need = j.offset + j.n * pcm.bytes_per_frame(j.format, j.channels)
                if need > srcs[k].numel() or j.n > outs[k].numel():
                    raise ValueError(f"job {k}: {need} source bytes / {j.n} frames exceed its buffers")
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        self._chk(self.lib.sc_pcm_decode(tab_dev.data_ptr(), n, self._stream()), "sc_pcm_decode")
        torch.cuda.synchronize(dev)
        lv, after = (np.frombuffer(a.cpu().numpy().tobytes(), _LEVEL_DT) for a in (lv_d, after_d))
        samples = [o.cpu().numpy().view(np.float32) for o in outs]
        return samples, [_level_dict(lv[k]) for k in range(n)], [_level_dict(after[k]) for k in range(n)]

    # ------------------------------------------------------------------
    def search_struct(self, sb):
        cached = getattr(sb, "_sc_search_struct", None)
        if cached is not None:
            return cached[0]
        w, cfg = sb.w, sb.cfg
        layers = (_abi.DecLayer * len(w.dec))()
        for i, lw in enumerate(w.dec):
            for name, _ in _abi.DecLayer._fields_:
                setattr(layers[i], name, lw[name].data_ptr() if name in lw else None)
        s = _abi.Search()
        s.S, s.W, s.K, s.V, s.d, s.H, s.F = sb.S, sb.W, sb.K, cfg.vocab_size, cfg.d_model, cfg.dec_heads, cfg.ffn_dim
        s.n_layers, s.TCAP, s.LCAP = cfg.dec_layers, sb.TCAP, sb.LCAP
        s.blank, s.eos, s.sos = cfg.blank_id, cfg.eos_id, cfg.sos_id
        s.w_dec, s.w_ctc, s.ln_eps = sb.search.decoder_weight, sb.search.ctc_weight, cfg.ln_eps
        for name in ("ctrl", "flags", "ctcx", "ckv", "skv", "yseq", "xpos", "anc", "score", "sc_dec",
                     "sc_ctc", "ctc_r", "ctc_rs", "ctc_s", "ctc_rnew", "dx", "dxn", "dqkv", "datt", "dq", "dffh",
                     "logits", "logp", "pre_ids", "psi", "psi_eos", "cand_score", "cand_tok", "cand_ctc",
                     "sel"):
            setattr(s, name, getattr(sb, name).data_ptr())
        s.embed, s.pe = w.embed.data_ptr(), w.pe.data_ptr()
        s.dec_norm_g, s.dec_norm_b = w.dec_norm_g.data_ptr(), w.dec_norm_b.data_ptr()
        s.out_w, s.out_b = w.out_w.data_ptr(), w.out_b.data_ptr()
        s.layers = C.cast(layers, C.c_void_p).value
        s.rowmap, s.n_rows = sb.rowmap.data_ptr(), sb.S * sb.W
        s.out_w_q = w.out_w_q.data_ptr() if getattr(w, "out_w_q", None) is not None else None
        s.kv_half = 1 if sb.ckv.dtype == torch.float16 else 0
        s.kv_rows, s.kvflags = int(sb.kv_rows), sb.kvflags.data_ptr()
        # fp16 decoder mode (weights.PackedWeights(dec_dtype="float16")): needs the fp16 K|V caches
        if s.kv_half and getattr(w, "out_w_qh", None) is not None and all("wqkv_pph" in lw for lw in w.dec):
            # layer projections | partial products (| 4: output layer, measured and rejected: csrc/streams.hip).  SC_ACT_HALF is a
            # test hook like every SC_* switch: honoured only under SC_TEST_HOOKS=1, exactly as the C++ engine reads it (sc_hook)
            hooks = os.environ.get("SC_TEST_HOOKS", "0") not in ("", "0")
            s.out_w_qh, s.act_half = w.out_w_qh.data_ptr(), (int(os.environ.get("SC_ACT_HALF", "3")) & 7) if hooks else 3
        else:
            for i in range(len(w.dec)):
                layers[i].wqkv_pph = layers[i].wq_pph = layers[i].wo_pph = layers[i].wo2_pph = None
        if getattr(sb, "ctcxT", None) is not None:  # column-major CTC table copy
            s.ctcxT, s.tct = sb.ctcxT.data_ptr(), sb.ctcxT.shape[-1]
        if getattr(sb, "ph1", None) is not None:   # head-parallel decoder layers (include/scasr.h)
            s.ph1, s.ph2, s.ffn_part = sb.ph1.data_ptr(), sb.ph2.data_ptr(), sb.ffn_part.data_ptr()
            s.max_ffn_part = sb.ffn_part.shape[0]
        sb._sc_search_struct = (s, layers)
        return s

    def _sb_call(self, fn, sb, *extra):
        s = self.search_struct(sb)
        s.n_rows = int(getattr(sb, "n_rows_step", sb.S * sb.W))   # compaction bucket of this step
        self._chk(getattr(self.lib, fn)(C.addressof(s), *extra, self._stream()), fn)

    def ctc_extend_state(self, sb):
        self._sb_call("sc_ctc_extend_state", sb)

    def dec_embed(self, sb):
        self._sb_call("sc_dec_embed", sb)

    def dec_self_attn(self, sb, li):
        self._sb_call("sc_dec_self_attn", sb, li)

    def dec_cross_attn(self, sb, li):
        self._sb_call("sc_dec_cross_attn", sb, li)

    def decoder_layers(self, sb):
        self._sb_call("sc_decoder_layers", sb)

    # head-parallel decoder layers: 3 launches per layer (csrc/decoder_layer.hip)
    def dec_layer_self(self, sb, li, xin, xout, npart):
        self._sb_call("sc_dec_layer_self", sb, li, _p(xin), _p(xout), _p(sb.ffn_part), int(npart))

    def dec_layer_cross(self, sb, li, xin, xout):
        self._sb_call("sc_dec_layer_cross", sb, li, _p(xin), _p(xout))

    def dec_layer_ffn(self, sb, li, xin, xout):
        n = C.c_int(0)
        self._sb_call("sc_dec_layer_ffn", sb, li, _p(xin), _p(xout), _p(sb.ffn_part), int(sb.ffn_part.shape[0]),
                      C.byref(n))
        return int(n.value)

    # stream-resident decoder layers: 2 launches per layer (csrc/decoder_stream.hip)
    def dec_layer_stream(self, sb, li, xin, xout, xn_out, npart):
        self._sb_call("sc_dec_layer_stream", sb, li, _p(xin), _p(xout), _p(xn_out), _p(sb.ffn_part), int(npart))

    def dec_layer_ffn_xn(self, sb, li, xn):
        n = C.c_int(0)
        self._sb_call("sc_dec_layer_ffn_xn", sb, li, _p(xn), _p(sb.ffn_part), int(sb.ffn_part.shape[0]), C.byref(n))
        return int(n.value)

    def dec_output_logits(self, sb, xin, xout, npart):
        self._sb_call("sc_dec_output_logits", sb, _p(xin), _p(xout), _p(sb.ffn_part), int(npart))

    def logsoftmax_topk(self, sb):
        self._sb_call("sc_logsoftmax_topk", sb)

    def ctc_prefix_scan(self, sb, split_min=0):
        """split_min > 0: streams with that many frames to walk take the T-parallel kernel (same scores)"""
        self._sb_call("sc_ctc_prefix_scan_split", sb, int(split_min))

    def fuse_topw(self, sb):
        self._sb_call("sc_fuse_topw", sb)

    def beam_prune(self, sb):
        self._sb_call("sc_beam_prune", sb)

    def ctc_gather_state(self, sb, split_min=0):
        """split_min: the value the step's ctc_prefix_scan ran with (streams split over T leave segment states, not checkpoints)"""
        self._sb_call("sc_ctc_gather_state_split", sb, int(split_min))

    def decode_step(self, sb):
        """One beam-search step; replayed from a hipGraph after the first call
        (all launch geometry depends only on S, W, V, TCAP, LCAP; the per-step
        state is read from the device-side ctrl rows)."""
        if not self.use_graphs:
            self._sb_call("sc_decode_step", sb)
            return
        graphs = getattr(sb, "_sc_decode_graphs", None)
        if graphs is None:
            graphs = sb._sc_decode_graphs = {}
        g = graphs.get(int(sb.n_rows_step))     # one graph per compaction bucket
        st = self._stream()
        if g is None:
            if st == 0:
                raise _abi.ScasrError("hipGraph capture needs a non-default stream (StreamBatch.stream)")
            self._sb_call("sc_decode_step", sb)          # warm-up launch (also validates arguments)
            self._chk(self.lib.sc_graph_capture_begin(st), "sc_graph_capture_begin")
            try:
                self._sb_call("sc_decode_step", sb)
            finally:
                out = C.c_void_p()
                rc = self.lib.sc_graph_capture_end(st, C.byref(out))
            self._chk(rc, "sc_graph_capture_end")
            graphs[int(sb.n_rows_step)] = out
            return self._redo_after_capture(sb)
        self._chk(self.lib.sc_graph_launch(g, st), "sc_graph_launch")

    def prepare_decode(self, sb):
        """Capture the decode-step graph of every compaction bucket up front
        (graph instantiation costs ~0.1 s per bucket; without this it would land
        in the middle of the stream the first time a bucket size occurs).  Runs
        dry steps: the device ctrl rows are all-inactive, so every per-stream
        kernel exits and the dense kernels only touch scratch activations."""
        if not self.use_graphs or self._stream() == 0:
            return
        keep = sb.n_rows_step
        for nb in range(sb.row_bucket, sb.S + sb.row_bucket, sb.row_bucket):
            sb.n_rows_step = min(nb, sb.S) * sb.W
            if int(sb.n_rows_step) not in getattr(sb, "_sc_decode_graphs", {}):
                self.decode_step(sb)
        sb.n_rows_step = keep

    def _redo_after_capture(self, sb):
        # the warm-up launch before capture already executed this step once;
        # kernels only write the 1-cur side, so the captured graph is NOT launched again here.
        return None
