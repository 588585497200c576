"""The stream-level C ABI of libscasr.so (include/scasr.h: sc_engine_* / sc_streams_* / sc_push / sc_submit / sc_poll /
sc_get_hyps_batch / sc_reset) behind the interface of ``engine.StreamBatch``: the whole state machine of the decoder - frontend and
encoder buffering, block schedule, beam-search step loop - runs in C++ (csrc/streams.hip); this file only
marshals arguments.  It is what ``Speech2TextStreaming`` / ``load_model`` / the scheduler use on a GPU.

``engine.StreamBatch`` is the same host logic in Python; it stays as the executable specification that runs on the
CPU spec backend against the reference fixtures.  Continuous batching (a stream's reply is ready when ITS blocks
are done, early streams start their next chunk while stragglers finish) is ``submit`` / ``poll`` here.
"""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .config import SearchConfig
from .engine import EngineError
from .weights import PackedWeights

_ERR_CAPACITY, _ERR_INPUT = -3, -4


class NativeEngine:
    """One weight replica on one GPU (sc_engine)."""

    def __init__(self, weights: Optional[PackedWeights] = None, packed_path: Optional[str] = None, device="cuda:0"):
        self.lib = _abi.load()
        self.device = torch.device(device)
        h = C.c_void_p()
        if packed_path is not None:
            _abi.check(self.lib.sc_engine_load(str(packed_path).encode(), self.device.index or 0, C.byref(h)),
                       "sc_engine_load")
            self.weights = None
        else:
            self.weights = weights            # keeps the device tensors alive: the engine borrows them
            cfg = weights.cfg
            c = _abi.Config()
            for n, _ in _abi.Config._fields_:
                setattr(c, n, weights.mvn_mode() if n == "mvn_mode" else getattr(cfg, n))
            ts = weights.named_tensors()
            self._names = [n.encode() for n, _ in ts]
            arr = (_abi.NamedTensor * len(ts))()
            for i, (n, t) in enumerate(ts):
                arr[i].name, arr[i].data, arr[i].numel = self._names[i], t.data_ptr(), t.numel()
                arr[i].dtype = {torch.float64: 1, torch.float16: 2}.get(t.dtype, 0)
            _abi.check(self.lib.sc_engine_create(C.byref(c), arr, len(ts), self.device.index or 0, C.byref(h)),
                       "sc_engine_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sc_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass


class _Info:
    __slots__ = ("_b", "_s")
    _MAP = {"T_enc": "enc_frames", "processed_block": "processed_block", "process_idx": "process_idx",
            "L": "hyp_len", "nhyp": "n_hyp", "n_steps_total": "decode_steps", "fe_started": "frontend_started",
            "pcm_buffered": "pcm_buffered"}

    def __init__(self, b, s):
        self._b, self._s = b, s

    def __getattr__(self, name):
        info = _abi.StreamInfo()
        _abi.check(self._b.lib.sc_stream_info(self._b.handle, self._s, C.byref(info)), "sc_stream_info")
        v = getattr(info, self._MAP[name])
        return bool(v) if name == "fe_started" else int(v)


class _InfoList:
    def __init__(self, b):
        self._b = b

    def __getitem__(self, s):
        return _Info(self._b, s)

    def __iter__(self):
        return (_Info(self._b, s) for s in range(self._b.S))

    def __len__(self):
        return self._b.S


class NativeStreamBatch:
    """S independent streams on one engine (sc_streams); interface of engine.StreamBatch."""

    def __init__(self, weights, n_streams: int, search: SearchConfig = SearchConfig(), max_frames: int = 1600,
                 max_tokens: int = 640, pcm_capacity: int = 1 << 20, max_chunk_samples: int = 32768,
                 strict_reference: bool = True, engine: Optional[NativeEngine] = None, kv_dtype: str = "float32",
                 kv_pool_rows: int = 0):
        """``kv_dtype``: "float32" (the reference's arithmetic) or "float16" - the self- and cross-attention K|V
        caches in fp16 (half the HBM stream of the attention kernels and half the cache memory; arithmetic,
        softmax and all scores stay fp32): the storage mode of BASELINE configs[4], opt-in, never the parity mode.
        ``kv_pool_rows``: rows of the self-attention K|V pool per stream and layer (0: one row per (position, hypothesis) -
        never exhausted before max_tokens - unless that takes more than a quarter of the free device memory, then what the
        budget holds, at least 1.5 x max_tokens + 4 x beam; a stream that needs more fails with a capacity error)."""
        if not torch.cuda.is_available():
            raise _abi.ScasrError("NativeStreamBatch needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.engine = engine or NativeEngine(weights, device=weights.device)
        self.lib = self.engine.lib
        self.w, self.cfg, self.search = weights, (weights.cfg if weights is not None else None), search
        self.S, self.W = n_streams, search.beam_size
        self.TCAP, self.LCAP, self.PCAP = max_frames, max_tokens, pcm_capacity
        self.strict_reference = strict_reference
        if search.pre_beam != 40 or search.max_length != 500:
            raise EngineError("the native engine implements the reference's constants: pre-beam 40, max_length 500")
        o = _abi.StreamOptions(n_streams, search.beam_size, search.ctc_weight, int(search.use_bbd), max_frames,
                               max_tokens, pcm_capacity, max_chunk_samples, int(strict_reference),
                               {"float32": 0, "float16": 1}[kv_dtype], int(kv_pool_rows))
        self.kv_dtype = kv_dtype
        h = C.c_void_p()
        try:
            _abi.check(self.lib.sc_streams_create(self.engine.handle, C.byref(o), C.byref(h)), "sc_streams_create")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        self.handle = h
        self.st = _InfoList(self)
        self._coded = {}   # stream -> (format, channels, channel, scale) of the streams with an input format

    # ---- StreamBatch interface ---------------------------------------------------------------------
    @property
    def stats(self):
        a, b, c = C.c_long(), C.c_long(), C.c_long()
        self.lib.sc_streams_stats(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return {"enc_calls": a.value, "dec_steps": b.value, "dec_blocks": c.value}

    def _fault(self, s, code):
        msg = (self.lib.sc_stream_last_error(self.handle, int(s)) or b"").decode()
        return (RuntimeError if code == _ERR_INPUT else EngineError)(f"stream {s}: {msg}")

    @staticmethod
    def _marshal(ids, ptrs, counts, finals):
        n = len(ids)
        return ((C.c_int32 * n)(*ids), (C.c_void_p * n)(*ptrs), (C.c_int32 * n)(*counts),
                (C.c_uint8 * n)(*[1 if f else 0 for f in finals]))

    def _call(self, fn, ids, ptrs, counts, finals, keep, isolate_faults):
        n = len(ids)
        a_ids, a_ptr, a_cnt, a_fin = self._marshal(ids, ptrs, counts, finals)
        status = (C.c_int32 * n)()
        try:
            _abi.check(getattr(self.lib, fn)(self.handle, a_ids, a_ptr, a_cnt, a_fin, n, status), fn)
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        del keep
        out = {}
        for i, s in enumerate(ids):
            if status[i] >= 0:
                out[s] = bool(status[i])
                continue
            exc = self._fault(s, status[i])
            if not isolate_faults:
                raise exc     # the other streams of the call were decoded; this one has been reset
            out[s] = exc
        return out

    def _gather(self, chunks, pcm_resident):
        ids, ptrs, counts, finals, keep = [], [], [], [], []
        for s, samples, fin in chunks:
            ids.append(int(s))
            finals.append(bool(fin))
            if pcm_resident:
                ptrs.append(None)
                counts.append(int(samples))
            elif int(s) in self._coded:
                a, n = self._coded_bytes(int(s), samples)
                keep.append(a)
                ptrs.append(a.ctypes.data if a.size else None)
                counts.append(n)
            else:
                if isinstance(samples, torch.Tensor):
                    samples = samples.detach().cpu().numpy()
                a = np.ascontiguousarray(samples, dtype=np.float32)
                keep.append(a)
                ptrs.append(a.ctypes.data)
                counts.append(int(a.shape[0]))
        return ids, ptrs, counts, finals, keep

    def _coded_bytes(self, s, samples):
        """the chunk of a stream with an input format -> (contiguous uint8 array, sample frames): bytes, bytearray,
        memoryview or an array whose bytes are the codes (integer dtypes; float32 for the f32 format)"""
        from . import pcm
        fmt, channels, _, _ = self._coded[s]
        if isinstance(samples, torch.Tensor):
            samples = samples.detach().cpu().numpy()
        if isinstance(samples, np.ndarray) and samples.dtype.kind == "f" and not (fmt == pcm.F32 and samples.dtype == np.float32):
            raise EngineError(f"stream {s} has input format {pcm.NAME_OF[fmt]}: it takes the coded bytes, not {samples.dtype} samples")
        a = np.ascontiguousarray(pcm.as_bytes(samples))
        bpf = pcm.bytes_per_frame(fmt, channels)
        if a.size % bpf:
            raise EngineError(f"stream {s}: {a.size} bytes are not a whole number of {bpf}-byte frames")
        return a, a.size // bpf

    def push(self, chunks: Sequence[Tuple[int, Optional[np.ndarray], bool]], pcm_resident: bool = False,
             isolate_faults: bool = False):
        """One chunk step: (stream, samples, is_final); with ``pcm_resident`` the tuple carries the sample COUNT
        and the samples already sit in the device PCM ring (write_pcm).  A stream with an input format
        (``set_input_format``) takes its coded bytes: bytes, memoryview or an integer array.  Returns
        {stream: has_output}; a stream that failed carries its exception instead when ``isolate_faults`` (else it is
        raised)."""
        ids, ptrs, counts, finals, keep = self._gather(chunks, pcm_resident)
        fn = "sc_push_raw" if any(s in self._coded for s in ids) else "sc_push"
        return self._call(fn, ids, ptrs, counts, finals, keep, isolate_faults)

    def push_raw(self, chunks, isolate_faults: bool = False):
        """``push`` through sc_push_raw whatever the streams' formats (floats for a stream without one)"""
        ids, ptrs, counts, finals, keep = self._gather(chunks, False)
        return self._call("sc_push_raw", ids, ptrs, counts, finals, keep, isolate_faults)

    def push_block(self, stream_ids: np.ndarray, pcm: np.ndarray, finals: Optional[np.ndarray] = None) -> np.ndarray:
        """sc_push for row i of a contiguous float32 matrix ``pcm`` [n, samples] -> stream ``stream_ids[i]`` without
        per-chunk Python work (the batched callers: bench, scheduler).  Returns the int32 status array (sc_push)."""
        n, m = pcm.shape
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and len(stream_ids) == n
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        ptrs = (pcm.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(m * 4)).astype(np.uint64)
        cnt = np.full(n, m, np.int32)
        fin = np.zeros(n, np.uint8) if finals is None else np.ascontiguousarray(finals, dtype=np.uint8)
        status = np.zeros(n, np.int32)
        _abi.check(self.lib.sc_push(self.handle, ids.ctypes.data_as(_abi.c_int_p), ptrs.ctypes.data_as(C.POINTER(C.c_void_p)),
                                    cnt.ctypes.data_as(_abi.c_int_p), fin.ctypes.data_as(C.POINTER(C.c_uint8)), n,
                                    status.ctypes.data_as(_abi.c_int_p)), "sc_push")
        return status

    # ---- continuous batching (sc_submit / sc_poll) ---------------------------------------------------
    def submit(self, chunks: Sequence[Tuple[int, Optional[np.ndarray], bool]], pcm_resident: bool = False, raw: bool = False):
        """Hand the engine one chunk per listed stream and return at once (the chunks are copied); their frontend +
        encoder stage is issued as one group.  A stream's next chunk may be submitted once ``poll`` has reported
        this one."""
        ids, ptrs, counts, finals, keep = self._gather(chunks, pcm_resident)
        fn = "sc_submit_raw" if raw or any(s in self._coded for s in ids) else "sc_submit"
        a_ids, a_ptr, a_cnt, a_fin = self._marshal(ids, ptrs, counts, finals)
        try:
            _abi.check(getattr(self.lib, fn)(self.handle, a_ids, a_ptr, a_cnt, a_fin, len(ids)), fn)
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        del keep

    def submit_raw(self, chunks):
        """``submit`` through sc_submit_raw whatever the streams' formats (floats for a stream without one)"""
        self.submit(chunks, raw=True)

    def submit_block(self, stream_ids: np.ndarray, pcm: np.ndarray, finals: Optional[np.ndarray] = None):
        n, m = pcm.shape
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and len(stream_ids) == n
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        ptrs = (pcm.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(m * 4)).astype(np.uint64)
        cnt = np.full(n, m, np.int32)
        fin = np.zeros(n, np.uint8) if finals is None else np.ascontiguousarray(finals, dtype=np.uint8)
        _abi.check(self.lib.sc_submit(self.handle, ids.ctypes.data_as(_abi.c_int_p), ptrs.ctypes.data_as(C.POINTER(C.c_void_p)),
                                      cnt.ctypes.data_as(_abi.c_int_p), fin.ctypes.data_as(C.POINTER(C.c_uint8)), n), "sc_submit")

    def poll(self, min_done: int = 1, isolate_faults: bool = True):
        """Run the engine until at least ``min_done`` outstanding chunks are complete (or none is outstanding).
        Returns {stream: has_output | exception} for the chunks reported by this call."""
        ids = np.zeros(self.S, np.int32)
        st = np.zeros(self.S, np.int32)
        n = self.lib.sc_poll(self.handle, int(min_done), self.S, ids.ctypes.data_as(_abi.c_int_p), st.ctypes.data_as(_abi.c_int_p))
        if n < 0:
            _abi.check(n, "sc_poll")
        out = {}
        for i in range(n):
            s = int(ids[i])
            if st[i] >= 0:
                out[s] = bool(st[i])
            else:
                exc = self._fault(s, int(st[i]))
                if not isolate_faults:
                    raise exc
                out[s] = exc
        return out

    def poll_ids(self, min_done: int = 1, max_done: int = 0):
        """``poll`` without Python objects: (stream ids, statuses) as int32 arrays; at most ``max_done`` replies
        (0: all that are ready), oldest completion first."""
        ids = np.zeros(self.S, np.int32)
        st = np.zeros(self.S, np.int32)
        n = self.lib.sc_poll(self.handle, int(min_done), int(max_done) if max_done > 0 else self.S,
                             ids.ctypes.data_as(_abi.c_int_p), st.ctypes.data_as(_abi.c_int_p))
        if n < 0:
            _abi.check(n, "sc_poll")
        return ids[:n], st[:n]

    def set_encoder_batch(self, min_streams: int):
        """continuous batching: the encoder stages of successive admissions are issued as one group when it holds this
        many streams (or as soon as a decode block needs its frames); results do not depend on it"""
        _abi.check(self.lib.sc_streams_set_encoder_batch(self.handle, int(min_streams)), "sc_streams_set_encoder_batch")

    def set_queue_depth(self, depth: int):
        """chunks a stream may have outstanding (default 1: call -> reply -> next call).  depth > 1: ``submit`` accepts the
        next chunk(s) of a stream while an earlier one is still decoding (file / backlog hosts: the encoder of chunk k+1
        runs beside the decoding of chunk k); chunks are reported in order, one per ``poll`` and stream, with the same
        results, and the hypotheses of a reported chunk stay readable until the next ``poll``"""
        _abi.check(self.lib.sc_streams_set_queue_depth(self.handle, int(depth)), "sc_streams_set_queue_depth")
        self.queue_depth = int(depth)

    @property
    def outstanding(self) -> int:
        return int(self.lib.sc_streams_outstanding(self.handle))

    def push_features(self, items, isolate_faults: bool = False):
        ids, ptrs, counts, finals, keep = [], [], [], [], []
        for s, feats, fin in items:
            if isinstance(feats, torch.Tensor):
                feats = feats.detach().cpu().numpy()
            a = np.ascontiguousarray(feats, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != self.cfg.n_mels:
                raise EngineError(f"features must be (T, {self.cfg.n_mels})")
            keep.append(a)
            ids.append(int(s)); ptrs.append(a.ctypes.data); counts.append(int(a.shape[0])); finals.append(bool(fin))
        return self._call("sc_push_features", ids, ptrs, counts, finals, keep, isolate_faults)

    def reset(self, s: int):
        _abi.check(self.lib.sc_reset(self.handle, int(s)), "sc_reset")

    def set_input_rate(self, s: int, rate: int):
        """Rate of the samples ``push`` / ``submit`` take for stream s (default 16000; any rate of
        speechcatcher_amd.resample): converted to 16 kHz on the GPU in the admission's staging step.  Only on an idle
        stream that has buffered nothing since its last reset; ``reset`` keeps the rate."""
        try:
            _abi.check(self.lib.sc_stream_set_input_rate(self.handle, int(s), int(rate)), "sc_stream_set_input_rate")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def input_rate(self, s: int) -> int:
        return int(self.lib.sc_stream_input_rate(self.handle, int(s)))

    def set_input_format(self, s: int, format: int = 0, channels: int = 1, channel: int = -1, scale: int = 0):
        """Wire format of the audio ``push`` / ``submit`` take for stream s (speechcatcher_amd.pcm: F32 .. ALAW, 1..8
        interleaved channels, one channel or pcm.MIX, pcm.SCALE_FULL / SCALE_SERVER): decoded on the GPU in the admission's
        staging step, before the copy / sample-rate conversion.  Only on an idle stream that has buffered nothing since
        its last reset; ``reset`` keeps the format.  (F32, 1 channel) is the default: float samples, no decode launch."""
        from . import pcm
        try:
            _abi.check(self.lib.sc_stream_set_input_format(self.handle, int(s), int(format), int(channels), int(channel),
                                                           int(scale)), "sc_stream_set_input_format")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        if int(format) != pcm.F32 or int(channels) != 1:
            self._coded[int(s)] = (int(format), int(channels), int(channel), int(scale))
        else:
            self._coded.pop(int(s), None)

    def input_format(self, s: int):
        """-> (format, channels, channel, scale) of stream s"""
        v = [C.c_int32() for _ in range(4)]
        _abi.check(self.lib.sc_stream_input_format(self.handle, int(s), *[C.byref(x) for x in v]), "sc_stream_input_format")
        return tuple(int(x.value) for x in v)

    def input_level(self, s: int) -> dict:
        """cumulative input level of stream s up to and including its last reported chunk (pcm.LEVEL_FIELDS)"""
        lv = _abi.InputLevel()
        _abi.check(self.lib.sc_stream_input_level(self.handle, int(s), C.byref(lv)), "sc_stream_input_level")
        return {f: int(getattr(lv, f)) for f in _abi.LEVEL_FIELDS}

    def reset_all(self):
        for s in range(self.S):
            self.reset(s)

    def hypotheses_arrays(self, streams: Sequence[int], nbest: Optional[int] = None):
        """Live hypotheses of the listed streams with ONE device round trip (sc_get_hyps_batch): numpy arrays
        ids / xpos [n, nbest, Lmax], lens / scores / score_dec / score_ctc [n, nbest], n_hyps [n]."""
        nb = self.W if nbest is None else int(nbest)
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        # (queue depth > 1: the copies taken at completion may be longer than the stream's live hypotheses)
        lmax = max([1] + [self.st[int(s)].L for s in sid]) if n <= 4 and getattr(self, "queue_depth", 1) <= 1 else self.LCAP
        ids = np.zeros((n, nb, lmax), np.int32)
        xp = np.zeros((n, nb, lmax), np.int32)
        lens = np.zeros((n, nb), np.int32)
        nh = np.zeros(n, np.int32)
        sc, sd, scc = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb))
        ip, dp = _abi.c_int_p, _abi.c_double_p
        _abi.check(self.lib.sc_get_hyps_batch(self.handle, sid.ctypes.data_as(ip), n, nb, lmax, ids.ctypes.data_as(ip),
                                              xp.ctypes.data_as(ip), lens.ctypes.data_as(ip), nh.ctypes.data_as(ip),
                                              sc.ctypes.data_as(dp), sd.ctypes.data_as(dp), scc.ctypes.data_as(dp)),
                   "sc_get_hyps_batch")
        return {"ids": ids, "xpos": xp, "lens": lens, "n_hyps": nh, "score": sc, "score_dec": sd, "score_ctc": scc}

    def align(self, streams: Sequence[int], nbest: Optional[int] = None):
        """CTC forced alignment of the hypotheses hypotheses_arrays reports, best first (sc_align_hyps), against the
        stream's CTC rows of the decode block they come from.  Labels: yseq without <sos> and a trailing <eos>.
        numpy arrays start / end (exclusive) [n, nbest, Lmax] in encoder frames, logp_mean [n, nbest, Lmax],
        path_score / status [n, nbest] (status: _abi.ALIGN_*), n_hyps [n]; entries past a hypothesis' label count
        are undefined (labels = lens - 1, or - 2 when the hypothesis ends with <eos>)."""
        nb = self.W if nbest is None else int(nbest)
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        lmax = self.LCAP
        start = np.zeros((n, nb, lmax), np.int32)
        end = np.zeros((n, nb, lmax), np.int32)
        lp = np.zeros((n, nb, lmax), np.float32)
        ps = np.zeros((n, nb))
        st = np.zeros((n, nb), np.int32)
        nh = np.zeros(n, np.int32)
        ip = _abi.c_int_p
        _abi.check(self.lib.sc_align_hyps(self.handle, sid.ctypes.data_as(ip), n, nb, lmax, start.ctypes.data_as(ip),
                                          end.ctypes.data_as(ip), lp.ctypes.data_as(_abi.c_float_p),
                                          ps.ctypes.data_as(_abi.c_double_p), st.ctypes.data_as(ip),
                                          nh.ctypes.data_as(ip)), "sc_align_hyps")
        return {"start": start, "end": end, "logp_mean": lp, "path_score": ps, "status": st, "n_hyps": nh}

    def alternates(self, streams: Sequence[int], nbest: Optional[int] = None, k: int = 3):
        """``align`` and, for every token of every hypothesis, its ``k`` acoustic alternates (sc_alternates_hyps; DESIGN.md
        8h): the alignment's arrays exactly as ``align`` returns them, plus alt_ids [n, nbest, Lmax, k] (-1: no such
        candidate), alt_logp [n, nbest, Lmax, k] float64 (mean log-posterior over the token's frames), own_rank
        [n, nbest, Lmax] (candidates ahead of the token itself; 0: it is the acoustic best of its frames) and span_status
        [n, nbest, Lmax] (_abi.ALT_*).  One call, one copy back; entries past a hypothesis' label count are undefined."""
        nb = self.W if nbest is None else int(nbest)
        k = int(k)
        if not 1 <= k <= _abi.ALT_MAX_K:
            raise ValueError(f"k must be in [1, {_abi.ALT_MAX_K}]")
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        lmax = self.LCAP
        start = np.zeros((n, nb, lmax), np.int32)
        end = np.zeros((n, nb, lmax), np.int32)
        lp = np.zeros((n, nb, lmax), np.float32)
        ps = np.zeros((n, nb))
        st = np.zeros((n, nb), np.int32)
        nh = np.zeros(n, np.int32)
        ai = np.full((n, nb, lmax, k), -1, np.int32)
        al = np.full((n, nb, lmax, k), -np.inf)
        rk = np.full((n, nb, lmax), -1, np.int32)
        ss = np.full((n, nb, lmax), _abi.ALT_NO_SPAN, np.int32)
        ip, dp = _abi.c_int_p, _abi.c_double_p
        _abi.check(self.lib.sc_alternates_hyps(self.handle, sid.ctypes.data_as(ip), n, nb, lmax, k,
                                               start.ctypes.data_as(ip), end.ctypes.data_as(ip),
                                               lp.ctypes.data_as(_abi.c_float_p), ps.ctypes.data_as(dp),
                                               st.ctypes.data_as(ip), ai.ctypes.data_as(ip), al.ctypes.data_as(dp),
                                               rk.ctypes.data_as(ip), ss.ctypes.data_as(ip), nh.ctypes.data_as(ip)),
                   "sc_alternates_hyps")
        return {"start": start, "end": end, "logp_mean": lp, "path_score": ps, "status": st, "n_hyps": nh,
                "alt_ids": ai, "alt_logp": al, "own_rank": rk, "span_status": ss}

    def align_tokens(self, s: int, ids: Sequence[int]):
        """CTC forced alignment of a given transcript (token ids, no <sos> / <eos>) against the frames of stream s's
        reported hypotheses (sc_align_tokens): {"start", "end", "logp_mean": [L] arrays, "path_score", "status"}."""
        y = np.ascontiguousarray(ids, dtype=np.int32)
        L = y.shape[0]
        start, end = np.zeros(max(L, 1), np.int32), np.zeros(max(L, 1), np.int32)
        lp = np.zeros(max(L, 1), np.float32)
        ps, st = C.c_double(0.0), C.c_int32(0)
        ip = _abi.c_int_p
        _abi.check(self.lib.sc_align_tokens(self.handle, int(s), y.ctypes.data_as(ip), L, start.ctypes.data_as(ip),
                                            end.ctypes.data_as(ip), lp.ctypes.data_as(_abi.c_float_p), C.byref(ps),
                                            C.byref(st)), "sc_align_tokens")
        return {"start": start[:L], "end": end[:L], "logp_mean": lp[:L], "path_score": ps.value, "status": st.value}

    def read_ctc(self, s: int) -> np.ndarray:
        """Test aid: the CTC rows sc_align_hyps / align_tokens align stream s against -> [T, vocab] (sc_streams_read_ctc)."""
        a = np.zeros((self.TCAP, self.cfg.vocab_size), np.float32)
        T = self.lib.sc_streams_read_ctc(self.handle, int(s), a.ctypes.data, self.TCAP)
        if T < 0:
            _abi.check(T, "sc_streams_read_ctc")
        return a[:T].copy()

    def read_ctc_projected(self, s: int) -> np.ndarray:
        """Test aid: the CTC rows projected for stream s's utterance so far, as the device holds them now -> [T, vocab]
        (sc_streams_read_ctc_projected); raw logits for a decoder-free stream."""
        a = np.zeros((self.TCAP, self.cfg.vocab_size), np.float32)
        T = self.lib.sc_streams_read_ctc_projected(self.handle, int(s), a.ctypes.data, self.TCAP)
        if T < 0:
            _abi.check(T, "sc_streams_read_ctc_projected")
        return a[:T].copy()

    # ---- acoustic activity (sc_streams_set_activity) -----------------------------------------
    def set_activity(self, on: bool, blank_threshold: float = 0.8):
        """Per-stream speech activity from the CTC table: when on, every admission group scans the CTC rows it projects
        (one extra launch per group) - a frame is silence iff its blank posterior exceeds ``blank_threshold`` (or the row
        is bad).  Off by default; only while no chunk is outstanding."""
        try:
            _abi.check(self.lib.sc_streams_set_activity(self.handle, int(bool(on)), float(blank_threshold)),
                       "sc_streams_set_activity")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def activity(self, streams: Sequence[int]):
        """{field: int32 array [n]} (n_frames, n_speech, n_bad, first_speech, last_speech, trail_silence) of the listed
        streams' last reported chunks - the chunks whose hypotheses ``hypotheses`` returns."""
        out = {k: np.zeros(len(streams), np.int32) for k in _abi.ACTIVITY_FIELDS}
        a = _abi.Activity()
        for i, s in enumerate(streams):
            _abi.check(self.lib.sc_stream_activity(self.handle, int(s), C.byref(a)), "sc_stream_activity")
            for k in _abi.ACTIVITY_FIELDS:
                out[k][i] = getattr(a, k)
        return out

    def read_activity(self, s: int) -> np.ndarray:
        """float64 [T]: the blank posterior of every CTC row the state of stream s's last reported chunk covers"""
        a = np.zeros(self.TCAP, np.float64)
        T = self.lib.sc_streams_read_activity(self.handle, int(s), a.ctypes.data, self.TCAP)
        if T < 0:
            _abi.check(T, "sc_streams_read_activity")
        return a[:T].copy()

    # ---- phrase spotting (sc_streams_set_phrases) --------------------------------------------
    def set_phrases(self, phrases, min_scores=None):
        """Phrase spotting from the CTC table: ``phrases`` is a list of up to 64 token-id sequences (1..32 ids, no
        blank), ``min_scores`` their floors (default -2.0 per token).  With a set in place every admission group scans
        the CTC rows it projects (one extra launch per group); the search is not touched.  An empty list or None
        switches the option off (the default).  Only while no chunk is outstanding; every stream's state starts over."""
        from .spotting import PhraseSet
        try:
            if not phrases:
                _abi.check(self.lib.sc_streams_set_phrases(self.handle, None, None, None, 0), "sc_streams_set_phrases")
                self._phrases = None
                return
            ps = PhraseSet(phrases, min_scores, self.cfg.vocab_size, self.cfg.blank_id)
            _abi.check(self.lib.sc_streams_set_phrases(self.handle, ps.labels.ctypes.data, ps.lens.ctypes.data,
                                                       ps.floors.ctypes.data, ps.P), "sc_streams_set_phrases")
            self._phrases = ps
        except (_abi.ScasrError, ValueError) as e:
            raise EngineError(str(e)) from e

    def set_phrase_mask(self, s: int, mask: int):
        """bit p of ``mask``: phrase p is enabled for stream s (default: all); from the next chunk on"""
        try:
            _abi.check(self.lib.sc_stream_set_phrase_mask(self.handle, int(s), int(mask) & ((1 << 64) - 1)),
                       "sc_stream_set_phrase_mask")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def spot(self, streams: Sequence[int]):
        """{"n_frames", "n_events": int32 array [n]} of the listed streams' last reported chunks"""
        out = {k: np.zeros(len(streams), np.int32) for k in ("n_frames", "n_events")}
        a = _abi.Spot()
        for i, s in enumerate(streams):
            try:
                _abi.check(self.lib.sc_stream_spot(self.handle, int(s), C.byref(a)), "sc_stream_spot")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
            out["n_frames"][i], out["n_events"][i] = a.n_frames, a.n_events
        return out

    def spot_events(self, s: int):
        """[(end, phrase, start, score)]: the stored events (the utterance's first 64) the state of stream s's last
        reported chunk covers, ordered by (end, phrase); frames of the utterance, both inclusive"""
        ev = (_abi.SpotEvent * _abi.SPOT_MAX_EVENTS)()
        n = self.lib.sc_streams_read_spot_events(self.handle, int(s), C.addressof(ev), _abi.SPOT_MAX_EVENTS)
        if n < 0:
            try:
                _abi.check(n, "sc_streams_read_spot_events")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
        return [(e.end, e.phrase, e.start, e.score) for e in ev[:n]]

    def read_spot_state(self, s: int):
        """test aid: (values [P, 64] float64, starts [P, 64] int32) of stream s as the device holds them now"""
        P = self._phrases.P
        v, st = np.zeros((P, _abi.SPOT_STATES), np.float64), np.zeros((P, _abi.SPOT_STATES), np.int32)
        n = self.lib.sc_streams_read_spot_state(self.handle, int(s), v.ctypes.data, st.ctypes.data)
        if n < 0:
            _abi.check(n, "sc_streams_read_spot_state")
        return v, st

    # ---- draft transcript (sc_streams_set_draft) ---------------------------------------------
    def set_draft(self, on: bool = True):
        """Draft transcript from the CTC table: when on, every admission group runs the greedy collapse over the CTC rows
        it projects (one extra launch per group); the search is not touched.  Off by default; only while no chunk is
        outstanding; every stream's state starts over."""
        try:
            _abi.check(self.lib.sc_streams_set_draft(self.handle, int(bool(on))), "sc_streams_set_draft")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def draft(self, streams: Sequence[int]):
        """{field: array [n]} (speechcatcher_amd.draft.FIELDS; int32, open_conf float64) of the listed streams' last
        reported chunks - the chunks whose hypotheses ``hypotheses`` returns."""
        out = {k: np.zeros(len(streams), np.float64 if k == "open_conf" else np.int32) for k in _abi.DRAFT_FIELDS}
        a = _abi.Draft()
        for i, s in enumerate(streams):
            try:
                _abi.check(self.lib.sc_stream_draft(self.handle, int(s), C.byref(a)), "sc_stream_draft")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
            for k in _abi.DRAFT_FIELDS:
                out[k][i] = getattr(a, k)
        return out

    def draft_tokens(self, s: int):
        """[(id, start, end, conf)]: the draft the state of stream s's last reported chunk covers - the closed tokens,
        then the open one; frames of the utterance, both inclusive"""
        tk = (_abi.DraftToken * (self.TCAP + 1))()
        n = self.lib.sc_streams_read_draft(self.handle, int(s), C.addressof(tk), self.TCAP + 1)
        if n < 0:
            try:
                _abi.check(n, "sc_streams_read_draft")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
        return [(t.id, t.start, t.end, t.conf) for t in tk[:n]]

    def set_decoder(self, s: int, decoder: str = "full"):
        """Decoder mode of stream s: "full" (the default) or "ctc" - a decoder-free stream, served from its CTC rows alone
        (no decode blocks, no cross-attention K|V rows; everything else as for any stream).  Only on an idle stream that
        has taken nothing of its utterance; the mode outlives ``reset``."""
        mode = {"full": _abi.DECODER_FULL, "ctc": _abi.DECODER_NONE}[decoder]
        try:
            _abi.check(self.lib.sc_stream_set_decoder(self.handle, int(s), mode), "sc_stream_set_decoder")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def decoder(self, s: int) -> str:
        return "ctc" if self.lib.sc_stream_decoder(self.handle, int(s)) == _abi.DECODER_NONE else "full"

    # ---- CTC prefix beam search (sc_streams_set_ctc_beam) --------------------------------------
    def set_ctc_beam(self, beam: int = 8, candidates: int = 8):
        """CTC prefix beam search from the CTC table: with beam >= 1 every admission group searches the CTC rows it
        projects (one extra launch per group) with `beam` entries and `candidates` tokens per frame; the attention search
        is not touched.  beam = 0 switches it off (the default); only while no chunk is outstanding; every stream's state
        starts over."""
        try:
            _abi.check(self.lib.sc_streams_set_ctc_beam(self.handle, int(beam), int(candidates)), "sc_streams_set_ctc_beam")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def ctc_beam(self, streams: Sequence[int]):
        """[{n_frames, n_bad, n_nodes, entries: [(node, last, len, parent, pb, pnb)] best first}] of the listed streams'
        last reported chunks - the chunks whose hypotheses ``hypotheses`` returns."""
        out = []
        a = _abi.Beam()
        for s in streams:
            try:
                _abi.check(self.lib.sc_stream_ctc_beam(self.handle, int(s), C.byref(a)), "sc_stream_ctc_beam")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
            out.append({"n_frames": a.n_frames, "n_bad": a.n_bad, "n_nodes": a.n_nodes,
                        "entries": [(e.node, e.last, e.len, e.parent, e.pb, e.pnb)
                                    for e in a.e[:max(0, min(a.n_entries, _abi.BEAM_MAX))]]})
        return out

    def ctc_beam_hyps(self, streams: Sequence[int], nbest: int = 1, max_len: Optional[int] = None):
        """{stream: [{"ids", "frames", "pb", "pnb", "node", "status"}, best first]}: the first nbest entries of those
        states as token ids with the frames of their first emission - one launch and one copy back for all streams."""
        n, nbest = len(streams), min(int(nbest), _abi.BEAM_MAX)
        max_len = self.TCAP if max_len is None else int(max_len)
        ids_in = np.asarray(list(streams), np.int32)
        head = np.zeros((n, nbest, 4), np.int32)
        ids, frames = np.zeros((n, nbest, max_len), np.int32), np.zeros((n, nbest, max_len), np.int32)
        sc = np.zeros((n, nbest, 2), np.float64)
        try:
            _abi.check(self.lib.sc_ctc_beam_hyps(self.handle, ids_in.ctypes.data_as(_abi.c_int_p), n, nbest, max_len,
                                                 head.ctypes.data, ids.ctypes.data, frames.ctypes.data, sc.ctypes.data),
                       "sc_ctc_beam_hyps")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        out = {}
        for i, s in enumerate(streams):
            hy = []
            for r in range(nbest):
                L, status = int(head[i, r, 0]), int(head[i, r, 1])
                if status == _abi.BEAM_PACK_NO_ENTRY:
                    break
                L = max(0, min(L, max_len))
                hy.append({"ids": ids[i, r, :L].tolist(), "frames": frames[i, r, :L].tolist(), "pb": float(sc[i, r, 0]),
                           "pnb": float(sc[i, r, 1]), "node": int(head[i, r, 2]), "status": status})
            out[int(s)] = hy
        return out

    # ---- n-gram model fused into the CTC beam (sc_streams_set_ctc_beam_lm) ----------------------
    def set_ctc_beam_lm(self, model=None, alpha: float = 0.5, beta: float = 0.0):
        """Fuse a backoff n-gram model into the CTC prefix beam of every stream: ``model`` is a packed blob
        (speechcatcher_amd.ngram.pack, or the bytes of a .sclm file), a hip_backend.DeviceLm, or None to detach.  The
        beam then keeps its entries by total + alpha * lm + beta * len.  Needs set_ctc_beam; only while no chunk is
        outstanding; every stream's beam starts over.  ``alpha`` / ``beta`` are parameters, not tuned."""
        from .hip_backend import DeviceLm
        lm = None
        if model is not None:
            try:
                lm = model if isinstance(model, DeviceLm) else DeviceLm(self.lib, bytes(model))
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
        try:
            _abi.check(self.lib.sc_streams_set_ctc_beam_lm(self.handle, lm.handle if lm is not None else None,
                                                           float(alpha), float(beta)), "sc_streams_set_ctc_beam_lm")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        self._ctc_lm = lm   # (the engine reads the model on the device: it lives as long as it is attached)

    def ctc_beam_lm(self, streams: Sequence[int], nbest: int = _abi.BEAM_MAX):
        """[{"lm": [...], "ctx": [...], "fused": [...]}] beside ``ctc_beam``'s entries of the listed streams: the model's
        sum along each entry's prefix, the automaton's state after it, and the fused score the beam ranks by."""
        n, nbest = len(streams), min(int(nbest), _abi.BEAM_MAX)
        ids_in = np.asarray(list(streams), np.int32)
        fused = np.zeros((n, nbest), np.float64)
        out = []
        a = _abi.BeamLm()
        try:
            _abi.check(self.lib.sc_ctc_beam_hyps_lm(self.handle, ids_in.ctypes.data_as(_abi.c_int_p), n, nbest, None,
                                                    fused.ctypes.data), "sc_ctc_beam_hyps_lm")
            for i, s in enumerate(streams):
                _abi.check(self.lib.sc_stream_ctc_beam_lm(self.handle, int(s), C.byref(a)), "sc_stream_ctc_beam_lm")
                k = int(np.sum(~np.isnan(fused[i])))
                out.append({"lm": list(a.lm[:k]), "ctx": list(a.ctx[:k]), "fused": fused[i, :k].tolist()})
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return out

    # ---- a grammar per stream (sc_stream_set_grammar) -------------------------------------------
    def grammar(self, blob):
        """``blob`` (speechcatcher_amd.grammar.compile, the bytes of a .scgr file, or a hip_backend.DeviceGrammar) as a
        DeviceGrammar: validated and uploaded once; any number of streams, of any handle, may name it."""
        from .hip_backend import DeviceGrammar
        try:
            return blob if isinstance(blob, DeviceGrammar) else DeviceGrammar(self.lib, bytes(blob))
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def release_grammar(self, handle):
        """free a grammar() - an EngineError while a stream still names it"""
        try:
            handle.close()
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def set_stream_grammar(self, s: int, handle=None):
        """The grammar of stream s (a grammar(), or None: none): its CTC beam then answers only from it.  Needs
        set_ctc_beam and no model attached; only on an idle stream that has taken nothing of its utterance; the setting
        outlives ``reset``."""
        try:
            _abi.check(self.lib.sc_stream_set_grammar(self.handle, int(s), handle.handle if handle is not None else None),
                       "sc_stream_set_grammar")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        self._grammars = getattr(self, "_grammars", {})
        self._grammars[int(s)] = handle   # (the engine reads the grammar on the device: it lives while a stream names it)

    def ctc_beam_grammar(self, streams: Sequence[int]):
        """[[g, ...]] beside ``ctc_beam``'s entries of the listed streams: the grammar's state after each entry's prefix"""
        out = []
        a = _abi.BeamGr()
        for s, st in zip(streams, self.ctc_beam(streams)):
            try:
                _abi.check(self.lib.sc_stream_ctc_beam_grammar(self.handle, int(s), C.byref(a)), "sc_stream_ctc_beam_grammar")
            except _abi.ScasrError as e:
                raise EngineError(str(e)) from e
            out.append(list(a.g[:len(st["entries"])]))
        return out

    def ctc_beam_hyps_grammar(self, streams: Sequence[int], nbest: int = 1):
        """{stream: [(g, complete), best first]} beside ``ctc_beam_hyps``: the grammar's state after each entry and
        whether it accepts; (-1, None) for a stream without a grammar.  Host arithmetic, no launch."""
        n, nbest = len(streams), min(int(nbest), _abi.BEAM_MAX)
        ids_in = np.asarray(list(streams), np.int32)
        g, acc = np.zeros((n, nbest), np.int32), np.zeros((n, nbest), np.int32)
        try:
            _abi.check(self.lib.sc_ctc_beam_hyps_grammar(self.handle, ids_in.ctypes.data_as(_abi.c_int_p), n, nbest,
                                                         g.ctypes.data_as(_abi.c_int_p), acc.ctypes.data_as(_abi.c_int_p)),
                       "sc_ctc_beam_hyps_grammar")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return {int(s): [(int(g[i, r]), bool(acc[i, r]) if acc[i, r] >= 0 else None) for r in range(nbest)]
                for i, s in enumerate(streams)}

    def hypotheses_batch(self, streams: Sequence[int], nbest: Optional[int] = None):
        """{stream: [hypothesis dicts, best first]} for the listed streams, one device round trip for all."""
        a = self.hypotheses_arrays(streams, nbest)
        out = {}
        for i, s in enumerate(streams):
            hy = []
            for j in range(int(a["n_hyps"][i])):
                L = int(a["lens"][i, j])
                hy.append({"yseq": a["ids"][i, j, :L].tolist(), "score": float(a["score"][i, j]),
                           "score_dec": float(a["score_dec"][i, j]), "score_ctc": float(a["score_ctc"][i, j]),
                           "xpos": a["xpos"][i, j, :L].tolist()})
            out[int(s)] = hy
        return out

    def hyps_delta_arrays(self, streams: Sequence[int], from_: Sequence[int], final: Sequence[int] = ()):
        """sc_get_hyps_delta as numpy arrays, one device round trip for all listed streams: L / commit / n_hyps / status
        [n] int32, ids / xpos [n, max_tail] int32 and stability [n, max_tail] float64 (row i: its first L[i] - from_[i]
        entries; the rest is undefined), scores [n, 3] (total, decoder, ctc).  ``final``: the listed streams whose chunk was the utterance's last."""
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        frm = np.ascontiguousarray(from_, dtype=np.int32)
        n = len(sid)
        if frm.shape != (n,):
            raise ValueError("one from per stream")
        fin = np.zeros(n, np.int32)
        if len(final):
            fin[np.isin(sid, np.asarray(list(final), np.int32))] = 1
        mt = max(1, self.LCAP - (int(frm.min()) if n else 0))
        ints = np.zeros((4, n), np.int32)
        # (not zeroed: the call writes the tails, the rest of a row is never touched - nor its pages)
        tails = np.empty((2, n, mt), np.int32)
        stab, sc = np.empty((n, mt)), np.zeros((n, 3))
        ip, dp = _abi.c_int_p, _abi.c_double_p
        try:
            _abi.check(self.lib.sc_get_hyps_delta(self.handle, sid.ctypes.data_as(ip), n, frm.ctypes.data_as(ip),
                                                  fin.ctypes.data_as(ip), mt, ints[0].ctypes.data_as(ip),
                                                  ints[1].ctypes.data_as(ip), ints[2].ctypes.data_as(ip),
                                                  tails[0].ctypes.data_as(ip), tails[1].ctypes.data_as(ip),
                                                  stab.ctypes.data_as(dp), sc.ctypes.data_as(dp), ints[3].ctypes.data_as(ip)),
                       "sc_get_hyps_delta")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return {"L": ints[0], "commit": ints[1], "n_hyps": ints[2], "status": ints[3], "from": frm, "ids": tails[0],
                "xpos": tails[1], "stability": stab, "scores": sc}

    def hyps_delta(self, streams: Sequence[int], from_: Sequence[int], final: Sequence[int] = ()):
        """Stable partials (sc_get_hyps_delta): {stream: {"L", "commit", "tokens", "xpos", "stability",
        "score", "score_dec", "score_ctc", "n_hyp", "status"}} for the listed streams - of the hypotheses
        ``hypotheses_batch`` would return, the length L, the length ``commit`` of the prefix all live hypotheses share (no
        later chunk changes it), and the best hypothesis from token ``from_[i]`` on with the share of the beam's mass
        behind each of those tokens.  ``final``: the listed streams whose chunk was the utterance's last (everything is
        committed).  One launch and one copy back for all; only the tails travel.  The call changes nothing."""
        a = self.hyps_delta_arrays(streams, from_, final)
        out = {}
        for i, s in enumerate(streams):
            t = int(a["L"][i]) - int(a["from"][i]) if a["n_hyps"][i] else 0
            sc = a["scores"][i]
            out[int(s)] = {"L": int(a["L"][i]), "commit": int(a["commit"][i]), "tokens": a["ids"][i, :t],
                           "xpos": a["xpos"][i, :t], "stability": a["stability"][i, :t], "score": float(sc[0]),
                           "score_dec": float(sc[1]), "score_ctc": float(sc[2]), "n_hyp": int(a["n_hyps"][i]),
                           "status": int(a["status"][i])}
        return out

    # ---- n-gram rescoring of final n-best lists (sc_rescore_hyps, sc_lm_rescore_lists) -----------
    def language_model(self, model):
        """``model`` (a packed blob, the bytes of a .sclm file or a hip_backend.DeviceLm) as a DeviceLm"""
        from .hip_backend import DeviceLm
        try:
            return model if isinstance(model, DeviceLm) else DeviceLm(self.lib, bytes(model))
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e

    def rescore_hyps(self, streams: Sequence[int], model, alpha: float = 0.5, beta: float = 0.0, lm_eos: int = -1,
                     final: Sequence[int] = (), nbest: Optional[int] = None):
        """{stream: {"order", "fused", "lm", "eos_lm", "status"}} for the hypotheses ``hypotheses_batch`` would return
        (numpy arrays over those rows; order[r] is the row at rank r by fused = score + alpha * (lm + eos_lm) +
        beta * labels): one launch and one copy back for all listed streams, nothing of the engine changes.  ``model``:
        language_model(); ``lm_eos``: the id that stands for </s> in the model, applied to the streams in ``final``."""
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        nb = min(int(self.W if nbest is None else nbest), _abi.RESCORE_MAX_HYPS)
        fin = np.zeros(n, np.int32)
        if len(final):
            fin[np.isin(sid, np.asarray(list(final), np.int32))] = 1
        order, status, nh = np.zeros((n, nb), np.int32), np.zeros((n, nb), np.int32), np.zeros(n, np.int32)
        fused, lm, eos = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb))
        ip = _abi.c_int_p
        try:
            _abi.check(self.lib.sc_rescore_hyps(self.handle, sid.ctypes.data_as(ip), n, nb, model.handle, float(alpha),
                                                float(beta), int(lm_eos), fin.ctypes.data_as(ip), order.ctypes.data,
                                                fused.ctypes.data, lm.ctypes.data, eos.ctypes.data, status.ctypes.data,
                                                nh.ctypes.data_as(ip)), "sc_rescore_hyps")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return {int(s): {"order": order[i, :nh[i]], "fused": fused[i, :nh[i]], "lm": lm[i, :nh[i]],
                         "eos_lm": eos[i, :nh[i]], "status": status[i, :nh[i]]} for i, s in enumerate(sid)}

    def rescore_lists(self, lists, scores, model, alpha: float = 0.5, beta: float = 0.0, lm_eos: int = -1, state0=None):
        """The same for caller-given lists: ``lists[i]`` is a list of label sequences (at most 16), ``scores[i]`` their
        totals, ``state0[i]`` the automaton's state before the first label (default: the model's start).  Returns one
        dict per list: "order", "fused", "lm", "eos_lm", "status", "end_state"."""
        n = len(lists)
        nb = max([len(li) for li in lists] + [1])
        if nb > _abi.RESCORE_MAX_HYPS:
            raise ValueError(f"a list holds more than {_abi.RESCORE_MAX_HYPS} rows")
        ml = max([len(y) for li in lists for y in li] + [1])
        ids, lens = np.zeros((n, nb, ml), np.int32), np.zeros((n, nb), np.int32)
        sc, sizes = np.zeros((n, nb)), np.zeros(n, np.int32)
        for i, (li, ss) in enumerate(zip(lists, scores)):
            if len(li) != len(ss):
                raise ValueError("one score per row")
            sizes[i] = len(li)
            for r, y in enumerate(li):
                ids[i, r, :len(y)], lens[i, r], sc[i, r] = y, len(y), ss[r]
        st = None if state0 is None else np.ascontiguousarray(state0, dtype=np.int32)
        if st is not None and st.shape != (n,):
            raise ValueError("one state0 per list")
        order, status, end = (np.zeros((n, nb), np.int32) for _ in range(3))
        fused, lm, eos = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb))
        try:
            _abi.check(self.lib.sc_lm_rescore_lists(self.handle, model.handle, ids.ctypes.data, lens.ctypes.data,
                                                    sc.ctypes.data, sizes.ctypes.data_as(_abi.c_int_p), n, nb, ml,
                                                    None if st is None else st.ctypes.data, float(alpha), float(beta),
                                                    int(lm_eos), order.ctypes.data, fused.ctypes.data, lm.ctypes.data,
                                                    eos.ctypes.data, status.ctypes.data, end.ctypes.data),
                       "sc_lm_rescore_lists")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return [{"order": order[i, :k], "fused": fused[i, :k], "lm": lm[i, :k], "eos_lm": eos[i, :k],
                 "status": status[i, :k], "end_state": end[i, :k]} for i, k in enumerate(sizes)]

    # ---- attention rescoring of n-best lists at finals (sc_attention_rescore_beam / _lists) ---------
    def attention_rescore_beam(self, streams: Sequence[int], nbest: Optional[int] = None, w_att: float = 1.0,
                               w_ctc: float = 0.5, beta: float = 0.0):
        """{stream: {"order", "fused", "att", "ctc_score", "status"}} for the first ``nbest`` entries of the listed
        streams' reported CTC beams (the entries ``ctc_beam_hyps`` returns; numpy arrays over those entries): one
        teacher-forced pass of the attention decoder over the stream's encoder output, fused = w_ctc * ctc_score +
        w_att * att + beta * labels, order[r] the entry at rank r.  One call and one copy back for all listed streams;
        nothing of the engine changes.  The streams must be idle (their chunks reported)."""
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        nb = min(int(_abi.ATT_MAX_HYPS if nbest is None else nbest), _abi.ATT_MAX_HYPS)
        order, status, nh = np.zeros((n, nb), np.int32), np.zeros((n, nb), np.int32), np.zeros(n, np.int32)
        fused, att, ctc = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb))
        try:
            _abi.check(self.lib.sc_attention_rescore_beam(self.handle, sid.ctypes.data_as(_abi.c_int_p), n, nb, float(w_att),
                                                          float(w_ctc), float(beta), order.ctypes.data, fused.ctypes.data,
                                                          att.ctypes.data, ctc.ctypes.data, status.ctypes.data,
                                                          nh.ctypes.data_as(_abi.c_int_p)), "sc_attention_rescore_beam")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return {int(s): {"order": order[i, :nh[i]], "fused": fused[i, :nh[i]], "att": att[i, :nh[i]],
                         "ctc_score": ctc[i, :nh[i]], "status": status[i, :nh[i]]} for i, s in enumerate(sid)}

    def attention_rescore_lists(self, streams: Sequence[int], lists, scores, w_att: float = 1.0, w_ctc: float = 0.5,
                                beta: float = 0.0):
        """The same for caller-given lists: ``lists[i]`` is a list of label sequences (at most 16, no <sos> / <eos>)
        scored against the encoder output of ``streams[i]`` (FULL or decoder-free), ``scores[i]`` their first-pass
        totals.  Returns one dict per list: "order", "fused", "att", "status"."""
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(lists)
        if len(sid) != n or len(scores) != n:
            raise ValueError("one stream and one score list per list")
        nb = max([len(li) for li in lists] + [1])
        if nb > _abi.ATT_MAX_HYPS:
            raise ValueError(f"a list holds more than {_abi.ATT_MAX_HYPS} rows")
        ml = max([len(y) for li in lists for y in li] + [1])
        ids, lens = np.zeros((n, nb, ml), np.int32), np.zeros((n, nb), np.int32)
        sc, sizes = np.zeros((n, nb)), np.zeros(n, np.int32)
        for i, (li, ss) in enumerate(zip(lists, scores)):
            if len(li) != len(ss):
                raise ValueError("one score per row")
            sizes[i] = len(li)
            for r, y in enumerate(li):
                ids[i, r, :len(y)], lens[i, r], sc[i, r] = y, len(y), ss[r]
        order, status = np.zeros((n, nb), np.int32), np.zeros((n, nb), np.int32)
        fused, att = np.zeros((n, nb)), np.zeros((n, nb))
        try:
            _abi.check(self.lib.sc_attention_rescore_lists(self.handle, sid.ctypes.data_as(_abi.c_int_p), n, ids.ctypes.data,
                                                           lens.ctypes.data, sc.ctypes.data,
                                                           sizes.ctypes.data_as(_abi.c_int_p), nb, ml, float(w_att),
                                                           float(w_ctc), float(beta), order.ctypes.data, fused.ctypes.data,
                                                           att.ctypes.data, status.ctypes.data),
                       "sc_attention_rescore_lists")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return [{"order": order[i, :k], "fused": fused[i, :k], "att": att[i, :k], "status": status[i, :k]}
                for i, k in enumerate(sizes)]

    def set_attention_rescore_workspace(self, max_bytes: int):
        """Upper bound of the workspace the two calls above allocate (default 256 MiB; include/scasr.h): a call that
        needs more runs in slabs of whole streams, with the same bits."""
        _abi.check(self.lib.sc_streams_set_attention_rescore_ws(self.handle, int(max_bytes)), "sc_streams_set_attention_rescore_ws")

    def attention_rescore_workspace(self):
        """(limit, allocated) bytes of that workspace; allocated is 0 until the first call"""
        lim, got = C.c_size_t(0), C.c_size_t(0)
        _abi.check(self.lib.sc_streams_attention_rescore_ws(self.handle, C.byref(lim), C.byref(got)), "sc_streams_attention_rescore_ws")
        return int(lim.value), int(got.value)

    # ---- consensus of final n-best lists (sc_mbr_hyps / sc_mbr_lists) ------------------------------------
    @staticmethod
    def _mbr_arrays(n: int, nb: int, ml: int):
        i32 = lambda *shape: np.zeros(shape, np.int32)     # noqa: E731
        return {"order": i32(n, nb), "risk": np.zeros((n, nb)), "weight": np.zeros((n, nb)), "status": i32(n, nb),
                "header": i32(n, 4), "dist": i32(n, 16, 16), "conf": np.zeros((n, ml)), "alt_tok": i32(n, ml),
                "alt_mass": np.zeros((n, ml)), "gap_mass": np.zeros((n, ml + 1))}

    @staticmethod
    def _mbr_entry(a, i: int, k: int):
        P, mp = int(a["header"][i, 0]), int(a["header"][i, 1])
        return {"order": a["order"][i, :k], "risk": a["risk"][i, :k], "weight": a["weight"][i, :k],
                "status": a["status"][i, :k], "pivot": P, "n_in": int(a["header"][i, 2]), "dist": a["dist"][i, :k, :k],
                "conf": a["conf"][i, :mp], "alt_tok": a["alt_tok"][i, :mp], "alt_mass": a["alt_mass"][i, :mp],
                "gap_mass": a["gap_mass"][i, :mp + 1] if P >= 0 else a["gap_mass"][i, :0]}

    def mbr_hyps(self, streams: Sequence[int], scale: float = 1.0, pivot_best: bool = False, nbest: Optional[int] = None):
        """{stream: consensus} for the hypotheses ``hypotheses_batch`` would return: the minimum-Bayes-risk row under
        the edit distance with weights softmax(scale * total), and the list's mass per slot of the pivot - "order"
        (rows by ascending risk), "risk", "weight", "status" (numpy arrays over those rows), "pivot" (the row; -1: none),
        "n_in", "dist", and per label of the pivot "conf", "alt_tok" (-1: nothing here; -2: no rival), "alt_mass", per gap
        "gap_mass".  ``pivot_best``: the pivot is row 0, the search's best.  One call and one copy back for all listed
        streams; nothing of the engine changes."""
        sid = np.ascontiguousarray(streams, dtype=np.int32)
        n = len(sid)
        nb = min(int(self.W if nbest is None else nbest), _abi.MBR_MAX_HYPS)
        ml = min(int(self.LCAP), _abi.MBR_MAX_LEN)
        a = self._mbr_arrays(n, nb, ml)
        nh = np.zeros(n, np.int32)
        try:
            _abi.check(self.lib.sc_mbr_hyps(self.handle, sid.ctypes.data_as(_abi.c_int_p), n, nb, float(scale),
                                            int(bool(pivot_best)), ml, a["order"].ctypes.data, a["risk"].ctypes.data,
                                            a["weight"].ctypes.data, a["status"].ctypes.data, a["header"].ctypes.data,
                                            a["dist"].ctypes.data, a["conf"].ctypes.data, a["alt_tok"].ctypes.data,
                                            a["alt_mass"].ctypes.data, a["gap_mass"].ctypes.data,
                                            nh.ctypes.data_as(_abi.c_int_p)), "sc_mbr_hyps")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return {int(s): self._mbr_entry(a, i, int(nh[i])) for i, s in enumerate(sid)}

    def mbr_lists(self, lists, values, weights: bool = False, scale: float = 1.0, pivots=None):
        """The same for caller-given lists: ``lists[i]`` is a list of label sequences (at most 16, no <sos> / <eos>),
        ``values[i]`` their totals - or, with ``weights``, their weights -, ``pivots[i]`` a row that is to be the pivot
        (default -1: the minimum-risk row).  Returns one dict per list, as mbr_hyps."""
        n = len(lists)
        if len(values) != n:
            raise ValueError("one value list per list")
        nb = max([len(li) for li in lists] + [1])
        if nb > _abi.MBR_MAX_HYPS:
            raise ValueError(f"a list holds more than {_abi.MBR_MAX_HYPS} rows")
        ml = max([len(y) for li in lists for y in li] + [1])
        ids, lens = np.zeros((n, nb, ml), np.int32), np.zeros((n, nb), np.int32)
        val, sizes = np.zeros((n, nb)), np.zeros(n, np.int32)
        for i, (li, vs) in enumerate(zip(lists, values)):
            if len(li) != len(vs):
                raise ValueError("one value per row")
            sizes[i] = len(li)
            for r, y in enumerate(li):
                ids[i, r, :len(y)], lens[i, r], val[i, r] = y, len(y), vs[r]
        pv = None if pivots is None else np.ascontiguousarray(pivots, dtype=np.int32)
        if pv is not None and pv.shape != (n,):
            raise ValueError("one pivot per list")
        a = self._mbr_arrays(n, nb, ml)
        try:
            _abi.check(self.lib.sc_mbr_lists(self.handle, ids.ctypes.data, lens.ctypes.data, val.ctypes.data, int(bool(weights)),
                                             sizes.ctypes.data_as(_abi.c_int_p), None if pv is None else pv.ctypes.data, n,
                                             nb, ml, float(scale), a["order"].ctypes.data, a["risk"].ctypes.data,
                                             a["weight"].ctypes.data, a["status"].ctypes.data, a["header"].ctypes.data,
                                             a["dist"].ctypes.data, a["conf"].ctypes.data, a["alt_tok"].ctypes.data,
                                             a["alt_mass"].ctypes.data, a["gap_mass"].ctypes.data), "sc_mbr_lists")
        except _abi.ScasrError as e:
            raise EngineError(str(e)) from e
        return [self._mbr_entry(a, i, int(k)) for i, k in enumerate(sizes)]

    def set_mbr_workspace(self, max_bytes: int):
        """Upper bound of the direction workspace the two calls above allocate (default 256 MiB, at least 8 MiB;
        include/scasr.h): a call that needs more runs in slabs of whole lists, with the same bits."""
        _abi.check(self.lib.sc_streams_set_mbr_ws(self.handle, int(max_bytes)), "sc_streams_set_mbr_ws")

    def mbr_workspace(self):
        """(limit, allocated) bytes of that workspace; allocated is 0 until the first call"""
        lim, got = C.c_size_t(0), C.c_size_t(0)
        _abi.check(self.lib.sc_streams_mbr_ws(self.handle, C.byref(lim), C.byref(got)), "sc_streams_mbr_ws")
        return int(lim.value), int(got.value)

    def hypotheses(self, s: int):
        """Live hypotheses of stream s: list of dicts (yseq, score, score_dec, score_ctc, xpos), best first."""
        return self.hypotheses_batch([int(s)])[int(s)]

    # ---- device-resident audio (bench) and the views of the drop-in class -------------------------------
    def write_pcm(self, s: int, offset: int, samples: np.ndarray):
        a = np.ascontiguousarray(samples, dtype=np.float32)
        _abi.check(self.lib.sc_streams_write_pcm(self.handle, int(s), int(offset), a.ctypes.data, a.shape[0]),
                   "sc_streams_write_pcm")

    def waveform_buffer(self, s: int) -> np.ndarray:
        n = self.st[s].pcm_buffered
        a = np.zeros(n, np.float32)
        if n:
            self.lib.sc_streams_read_pcm_buffer(self.handle, int(s), a.ctypes.data, n)
        return a

    def encoder_buffer(self, s: int) -> Optional[np.ndarray]:
        T = self.st[s].T_enc
        if T == 0:
            return None
        a = np.zeros((T, self.cfg.d_model), np.float32)
        self.lib.sc_streams_read_enc(self.handle, int(s), a.ctypes.data, T)
        return a

    def set_graphs(self, on: bool):
        self.lib.sc_streams_set_graphs(self.handle, int(bool(on)))

    def take_xattn_rows(self) -> int:
        return int(self.lib.sc_streams_take_xattn_rows(self.handle))

    def take_attn_counters(self):
        """{cross_rows, self_positions, self_distinct_rows}: [stand-alone kernels, head-parallel layer kernels, stream-resident
        layer kernel], summed over decode iterations, active streams and decoder layers since the last call"""
        r = (C.c_long * 9)()
        _abi.check(self.lib.sc_streams_take_attn_counters(self.handle, r), "sc_streams_take_attn_counters")
        return {"cross_rows": [int(r[0]), int(r[1]), int(r[2])], "self_positions": [int(r[3]), int(r[4]), int(r[5])],
                "self_distinct_rows": [int(r[6]), int(r[7]), int(r[8])]}

    def take_xattn_rows_by_kernel(self):
        """(rows read by the dec_attn_flash launches, by the sc_dec_layer_cross launches, by the sc_dec_layer_stream launches)"""
        r = (C.c_long * 3)()
        _abi.check(self.lib.sc_streams_take_xattn_rows_by_kernel(self.handle, r), "sc_streams_take_xattn_rows_by_kernel")
        return int(r[0]), int(r[1]), int(r[2])

    @property
    def kv_rows(self) -> int:
        """rows of the self-attention K|V pool per (stream, layer) this batch was created with"""
        return int(self.lib.sc_streams_kv_rows(self.handle))

    @property
    def hip_stream(self) -> int:
        return int(self.lib.sc_streams_hip_stream(self.handle) or 0)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sc_streams_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass
