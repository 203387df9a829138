"""Host-side mirror of include/sr_engine.h (ctypes over the C ABI of libsr_engine.so).

The shared library holds the hand-written gfx950 kernels; this module only moves pointers.
PyTorch is used for device memory and streams (plumbing).  There is no fallback: if the library is
missing, or no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsr_engine.so")
# the same sources built with -DSR_TESTING (csrc/Makefile): the development / test hooks of sr_dev_hook exist only there
TESTING_LIB_PATH = os.path.join(_HERE, "libsr_engine_testing.so")

DIS_ERR = 0xFFFFFFFF
ST_OK, ST_VAD_FAIL, ST_MFCC_FAIL, ST_SEG_OOB = 0, 1, 2, 3
N_COEF = 12
# per-frame intermediate values of the front end (sr_frame_features_batch*): packed FFT words, |X|*10, Mel energies, log*100
FEAT_FFT, FEAT_MAG, FEAT_MEL, FEAT_LOGMEL = 1, 2, 3, 4

RESULT_DTYPE = np.dtype([("best_tpl", "<u4"), ("min_dis", "<u4"), ("frm_num", "<u4"), ("status", "<u4")])
VAD_DTYPE = np.dtype([("mid_val", "<u4"), ("n_thl", "<u2"), ("z_thl", "<u2"), ("s_thl", "<u4"),
                      ("seg", "<i4", (6,)), ("frm_num", "<u4"), ("status", "<u4"), ("_pad", "<u4")])
ATAP_DTYPE = np.dtype([("mid_val", "<u4"), ("n_thl", "<u2"), ("z_thl", "<u2"), ("s_thl", "<u4")])
STREAM_SEG_DTYPE = np.dtype([("stream", "<u4"), ("start", "<i4"), ("end", "<i4"), ("frm_num", "<u4")])
# word-level N-best (sr_nbest_entry): a candidate word, its best slot, that slot's distance, its slots that matched at all
NBEST_DTYPE = np.dtype([("word", "<u4"), ("slot", "<u4"), ("dis", "<u4"), ("count", "<u4")])
NO_WORD, NBEST_MAX = 0xFFFFFFFF, 16
# live sessions (sr_live_seg): a segment of a channel, 64-bit sample offsets since the channel's recording began
LIVE_SEG_DTYPE = np.dtype([("channel", "<u4"), ("frm_num", "<u4"), ("start", "<i8"), ("end", "<i8")])
# word spotting (sr_spot_hit): q(e), the start and end frame of the best match inside a window, its accumulated cost
SPOT_DTYPE = np.dtype([("dis", "<u4"), ("start", "<u4"), ("end", "<u4"), ("acc", "<u4")])
# sr_spot_win: which (channel, window) an emitted row of a live spotting session holds
SPOT_WIN_DTYPE = np.dtype([("channel", "<u4"), ("window", "<u4")])
# full-DP alignment (sr_align_rec) and DBA training statistics (sr_train_stat)
ALIGN_DTYPE = np.dtype([("dis", "<u4"), ("acc", "<u4"), ("path_len", "<u4"), ("status", "<u4")])
TRAIN_STAT_DTYPE = np.dtype([("n_ok", "<u4"), ("n_fail", "<u4"), ("acc", "<u8")])
AL_OK, AL_GATED, AL_TOO_LONG, ALIGN_MAX_FRAMES = 0, 1, 2, 1024
# word-model clustering (sr_cluster_iter): one iteration's counters; CLUSTER_NONE = an example no model of its word admits
CLUSTER_ITER_DTYPE = np.dtype([("n_assigned", "<u4"), ("n_unassigned", "<u4"), ("n_moved", "<u4"), ("n_empty", "<u4"), ("acc", "<u8")])
CLUSTER_MAX, CLUSTER_NONE = 16, 0xFFFFFFFF
assert CLUSTER_ITER_DTYPE.itemsize == 24
# connected-word decoding (sr_chain_rec / sr_chain_word): a row's parse and its words in spoken order
CHAIN_REC_DTYPE = np.dtype([("cost", "<u4"), ("n_words", "<u4"), ("skipped", "<u4"), ("status", "<u4")])
CHAIN_WORD_DTYPE = np.dtype([("word", "<u4"), ("slot", "<u4"), ("start", "<u4"), ("end", "<u4"), ("acc", "<u4"), ("dis", "<u4"),
                             ("cum", "<u4"), ("reserved", "<u4")])
CH_OK, CH_NONE = 0, 1
CH_TRUNCATED = 2  # sr_decode_onepass_*: more words than words_cap, the first words_cap are written
OP_LIVE_TAIL = 1  # sr_onepass_live_open flag: the last words_cap words instead
# sr_vad_debug_masks: 16 words per capture, 63 frames (one round of the VAD kernel) per 64-bit word
VAD_MASK_WORDS, VAD_MASK_FRAMES = 16, 63
# sr_chain_live_row: which channel an emitted row of a live decoding session holds, and its frames after the push
CHAIN_LIVE_ROW_DTYPE = np.dtype([("channel", "<u4"), ("frames", "<u4")])
# sr_commit_rec: the committed words of a channel of a live one-pass session -- how many, how many of them earlier calls
# delivered, how many this call delivers, and the position below which every frame is decided
COMMIT_REC_DTYPE = np.dtype([("n_committed", "<u4"), ("first", "<u4"), ("n_new", "<u4"), ("frames", "<u4")])
assert COMMIT_REC_DTYPE.itemsize == 16
# sr_score_word_spans / sr_decode_words_alts modes: a span score row holds path costs, or costs / (L + M)
SPAN_ACC, SPAN_DIS = 0, 1
assert RESULT_DTYPE.itemsize == 16 and VAD_DTYPE.itemsize == 48 and SPOT_DTYPE.itemsize == 16
assert CHAIN_REC_DTYPE.itemsize == 16 and CHAIN_WORD_DTYPE.itemsize == 32 and CHAIN_LIVE_ROW_DTYPE.itemsize == 8
assert ALIGN_DTYPE.itemsize == 16 and TRAIN_STAT_DTYPE.itemsize == 16
assert ATAP_DTYPE.itemsize == 12 and STREAM_SEG_DTYPE.itemsize == 16 and NBEST_DTYPE.itemsize == 16
assert LIVE_SEG_DTYPE.itemsize == 24


class Config(C.Structure):
    _fields_ = [("fs", C.c_uint32), ("frame_time_ms", C.c_uint32), ("frame_mov_ms", C.c_uint32),
                ("nfft", C.c_uint32), ("n_mel", C.c_uint32), ("n_coef", C.c_uint32), ("max_frames", C.c_uint32),
                ("noise_len_ms", C.c_uint32), ("max_seg", C.c_uint32), ("device", C.c_int32)]


class SrError(RuntimeError):
    pass


_lib = None
_lib_testing = None


def _open(path):
    try:  # a process that also uses PyTorch must let torch load ITS HIP runtime first: libsr_engine.so then binds to the
        import torch  # noqa: F401  same libamdhip64 (loaded the other way round, torch finds "no HIP GPUs")
    except ImportError:
        pass
    if not os.path.exists(path):
        raise SrError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path)
    L.sr_last_error.restype = C.c_char_p
    L.sr_num_templates.restype = C.c_uint32
    L.sr_num_templates.argtypes = [C.c_void_p]
    L.sr_destroy.argtypes = [C.c_void_p]
    return L


def load_library(testing=False):
    """dlopen libsr_engine.so (built by __graft_entry__.build() / csrc/Makefile).  testing=True: the -DSR_TESTING build
    (libsr_engine_testing.so: development hooks compiled in), a second, independent library instance; the environment
    variable SR_ENGINE_TESTING=1 makes it the default of a whole process (test subprocesses that need hooks everywhere)."""
    global _lib, _lib_testing
    if testing or os.environ.get("SR_ENGINE_TESTING") == "1":
        if _lib_testing is None:
            _lib_testing = _open(TESTING_LIB_PATH)
            assert _lib_testing.sr_testing_build() == 1
        return _lib_testing
    if _lib is None:
        _lib = _open(os.environ.get("SR_ENGINE_LIB", LIB_PATH))  # development override: A/B-ing two builds on one GPU box
    return _lib


def _vp(x):
    """void* of a numpy array, a torch tensor, an int address or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


def dev_hook(name, value):
    """sr_dev_hook: development / test knobs (process-global, 0 = default); see include/sr_engine.h.  They exist only in
    the -DSR_TESTING build, so this always addresses libsr_engine_testing.so: engines that should see a hook are created
    with Engine(..., testing=True) / MultiEngine(..., testing=True) / Engine.clone(testing=True)."""
    L = load_library(testing=True)
    rc = L.sr_dev_hook(name.encode(), C.c_int64(value))
    if rc != 0:
        raise SrError(f"sr_dev_hook error {rc}: {L.sr_last_error().decode()}")


class _Tables(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("hamm", "tri_cen", "tri_even", "tri_odd", "dct", "tw_kr", "tw_ki", "log_thr")]


def build_tables(**kw):
    """Host-only sr_build_tables(): the constant tables sr_create generates for a configuration (no GPU touched).
    Keywords override sr_default_config fields (fs=16000, nfft=512, n_mel=40 for the extension front end)."""
    L = load_library()
    cfg = Config()
    L.sr_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    frame_len, nb = cfg.fs // 1000 * cfg.frame_time_ms, cfg.nfft // 2
    out = dict(hamm=np.zeros(frame_len, np.uint16), tri_cen=np.zeros(cfg.n_mel, np.uint16),
               tri_even=np.zeros(nb, np.uint16), tri_odd=np.zeros(nb, np.uint16),
               dct=np.zeros(cfg.n_coef * cfg.n_mel, np.int8), tw_kr=np.zeros(1020, np.int16),
               tw_ki=np.zeros(1020, np.int16), log_thr=np.zeros(2220, np.uint32))
    t = _Tables(**{k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()})
    rc = L.sr_build_tables(C.byref(cfg), C.byref(t))
    if rc != 0:
        raise SrError(f"sr_build_tables error {rc}: {L.sr_last_error().decode()}")
    out["tie_delta"] = np.zeros(32768, np.int8)  # front-end independent: its own entry point
    rc = L.sr_build_tie_table(out["tie_delta"].ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise SrError(f"sr_build_tie_table error {rc}: {L.sr_last_error().decode()}")
    return out


class Engine:
    """One sr_engine handle.  Defaults are the firmware's constants except where overridden."""

    def __init__(self, max_frames=119, device=-1, testing=False, **kw):
        self.L = load_library(testing)
        self._testing, self._kw, self._tpl = testing, dict(kw), None
        cfg = Config()
        self.L.sr_default_config(C.byref(cfg))
        cfg.max_frames = max_frames
        cfg.device = device
        for k, v in kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        self._check(self.L.sr_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_frames = max_frames
        self.n_coef = cfg.n_coef  # 12 except for the generic front end
        self.noise_len = (cfg.fs // 1000) * cfg.noise_len_ms

    @classmethod
    def borrowed(cls, handle, cfg, max_frames, lib=None):
        """a view of an sr_engine handle somebody else owns (sr_multi_engine): same methods, never destroyed from here"""
        e = cls.__new__(cls)
        e.L, e.cfg, e.h, e.max_frames, e._borrowed = lib if lib is not None else load_library(), cfg, C.c_void_p(handle), max_frames, True
        e._testing, e._kw, e._tpl = False, {}, None
        e.n_coef = cfg.n_coef
        e.noise_len = (cfg.fs // 1000) * cfg.noise_len_ms
        return e

    def clone(self, testing=False):
        """a second engine with this one's configuration and template store, on the product library or (testing=True) on
        the -DSR_TESTING build -- how a test points a development hook at the shapes of an engine it already has"""
        e = Engine(max_frames=self.max_frames, device=self.cfg.device, testing=testing, **self._kw)
        if self._tpl is not None:
            getattr(e, self._tpl[0])(*self._tpl[1])
        return e

    def _check(self, rc):
        if rc != 0:
            raise SrError(f"sr_engine error {rc}: {self.L.sr_last_error().decode()}")

    def mag_cheap_bound(self):
        """sr_mag_cheap_bound: 70171 when sr_create's sweep of this device confirmed the frame kernel's cheap magnitude form, else 0"""
        self.L.sr_mag_cheap_bound.restype = C.c_uint32
        return int(self.L.sr_mag_cheap_bound(self.h))

    def lds_poison(self, seed, stream=None):
        """sr_lds_poison: overwrite every CU's local data share with a seeded pattern; returns the bytes filled per workgroup"""
        n = C.c_uint32(0)
        self._check(self.L.sr_lds_poison(self.h, C.c_uint32(seed), C.c_void_p(stream), C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.sr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- template store ---------------------------------------------------------------------------
    @property
    def n_templates(self):
        return self.L.sr_num_templates(self.h)

    def set_templates_dense(self, mfcc, frames, valid=None):
        """mfcc int16 [K, rows, 12]; frames uint32 [K]; valid uint8 [K] or None (all valid)."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        if valid is not None:
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
        K = mfcc.shape[0]
        self._check(self.L.sr_set_templates_dense(self.h, _vp(mfcc), _vp(frames), _vp(valid), C.c_uint32(K),
                                                  C.c_uint32(mfcc.shape[1] * mfcc.shape[2])))
        self._tpl = ("set_templates_dense", (mfcc, frames, valid))

    def set_templates_store(self, store, stride=4096):
        """Firmware flash image: v_ftr_tag slots at `stride` bytes (Flash.H:11-20)."""
        store = np.ascontiguousarray(store, dtype=np.uint8)
        self._check(self.L.sr_set_templates(self.h, _vp(store), C.c_uint32(len(store) // stride), C.c_uint32(stride)))
        self._tpl = ("set_templates_store", (store, stride))

    def train_store(self, pcm, slots, store=None, n_slots=80, stride=4096):
        """save_mdl for each row of pcm into slot slots[i] of a flash-style store image (created erased,
        all 0xFF, when not given).  Returns (store uint8 [n_slots*stride], status uint32 [n])."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        n, S = pcm.shape
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        if store is None:
            store = np.full(n_slots * stride, 0xFF, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint32)
        self._check(self.L.sr_train_store(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(n), _vp(slots),
                                          _vp(store), C.c_uint32(len(store) // stride), C.c_uint32(stride), _vp(status)))
        return store, status

    # ---- words instead of slots ---------------------------------------------------------------------
    def set_word_map(self, words=None, slots_per_word=1):
        """sr_set_word_map: words uint32 [K] = one label per template slot (any value but NO_WORD), or None for the
        firmware's rule word = slot // slots_per_word (main.c:292).  The default map is word = slot."""
        if words is not None:
            words = np.ascontiguousarray(words, dtype=np.uint32)
        self._check(self.L.sr_set_word_map(self.h, _vp(words), C.c_uint32(0 if words is None else len(words)),
                                           C.c_uint32(slots_per_word)))
        self._wmap = (None if words is None else words.copy(), int(slots_per_word))  # (train_connected groups its examples by it)

    @staticmethod
    def word_groups(words=None, n_slots=None, slots_per_word=1):
        """Host-only sr_word_groups: the grouping of the slots by word that a map uploads.  Returns dict(order [n_slots],
        group_start [n_words + 1], word_id [n_words]) of uint32 arrays."""
        L = load_library()
        if words is not None:
            words = np.ascontiguousarray(words, dtype=np.uint32)
            n_slots = len(words)
        n_slots = int(n_slots or 0)
        order, start, ids = (np.zeros(n_slots, np.uint32), np.zeros(n_slots + 1, np.uint32), np.zeros(n_slots, np.uint32))
        nw = C.c_uint32(0)
        rc = L.sr_word_groups(_vp(words), C.c_uint32(n_slots), C.c_uint32(slots_per_word), _vp(order), _vp(start), _vp(ids),
                              C.byref(nw))
        if rc != 0:
            raise SrError(f"sr_word_groups error {rc}: {L.sr_last_error().decode()}")
        return dict(order=order, group_start=start[:nw.value + 1], word_id=ids[:nw.value])

    def nbest(self, scores, n_best):
        """sr_nbest_batch: scores uint32 [n_rows, K] (any score matrix of this store) -> (entries NBEST_DTYPE
        [n_rows, n_best], n_matched uint32 [n_rows]) under the engine's word map."""
        scores = np.ascontiguousarray(scores, dtype=np.uint32).reshape(-1, self.n_templates)
        n = scores.shape[0]
        nb = np.zeros((n, max(n_best, 0)), dtype=NBEST_DTYPE)
        nm = np.zeros(n, dtype=np.uint32)
        self._check(self.L.sr_nbest_batch(self.h, _vp(scores), C.c_uint32(n), C.c_uint32(n_best), _vp(nb), _vp(nm)))
        return nb, nm

    def nbest_dev(self, scores, n_best, stream=None):
        """sr_nbest_batch_dev on a device tensor of score rows int32 [n_rows, K] (contiguous).  Asynchronous; returns
        (entries int32 [n_rows, n_best, 4], n_matched int32 [n_rows]) device tensors."""
        import torch
        assert scores.is_cuda and scores.is_contiguous() and scores.shape[-1] == self.n_templates
        n = scores.numel() // self.n_templates
        if stream is None:
            stream = torch.cuda.current_stream(scores.device).cuda_stream
        nb = torch.empty(n, n_best, 4, dtype=torch.int32, device=scores.device)
        nm = torch.empty(n, dtype=torch.int32, device=scores.device)
        self._check(self.L.sr_nbest_batch_dev(self.h, _vp(scores), C.c_uint32(n), C.c_uint32(n_best), _vp(nb), _vp(nm),
                                              C.c_void_p(stream)))
        return nb, nm

    def rescore_nbest(self, mfcc, frames, nbest):
        """sr_rescore_nbest_dp, the second pass: mfcc int16 [n_rows, max_frames, 12], frames uint32 [n_rows], nbest NBEST_DTYPE
        [n_rows, n_best] (a first-pass list: nbest() of dtw() scores, or any list of candidate slots).  Every slot of every
        candidate word gets its full-DP score (dtw_dp's value) and the words are ranked again on the device.  Returns
        (entries NBEST_DTYPE [n_rows, n_best], n_rescored uint32 [n_rows])."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        nbest = np.ascontiguousarray(nbest, dtype=NBEST_DTYPE)
        n = mfcc.shape[0]
        nbest = nbest.reshape(n, -1)
        assert len(frames) == n
        out = np.zeros_like(nbest)
        nr = np.zeros(n, dtype=np.uint32)
        self._check(self.L.sr_rescore_nbest_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n),
                                               C.c_uint32(nbest.shape[1]), _vp(nbest), _vp(out), _vp(nr)))
        return out, nr

    def rescore_nbest_dev(self, mfcc, frames, nbest, frames_stride=1, stream=None):
        """sr_rescore_nbest_dp_dev on device tensors: mfcc int16 [n_rows, max_frames, 12]; nbest int32 [n_rows, n_best, 4];
        frames = a tensor (or view) whose first element is row 0's frame count, the next row's frames_stride 32-bit words
        further on: 1 for a plain int32 [n_rows], 4 for results[:, 2] and stream segment records, 6 for live segment records,
        12 for vad[:, 9].  Asynchronous; returns (entries int32 [n_rows, n_best, 4], n_rescored int32 [n_rows])."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and nbest.is_cuda and nbest.is_contiguous()
        n, n_best = nbest.shape[0], nbest.shape[1]
        assert mfcc.shape[0] == n
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        out = torch.empty(n, n_best, 4, dtype=torch.int32, device=mfcc.device)
        nr = torch.empty(n, dtype=torch.int32, device=mfcc.device)
        self._check(self.L.sr_rescore_nbest_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                   C.c_uint32(n_best), _vp(nbest), _vp(out), _vp(nr), C.c_void_p(stream)))
        return out, nr

    def recognize_nbest(self, pcm, n_best, want_scores=True, want_mfcc=True, want_vad=True, buf_len=None, rescore=False):
        """recognize() plus the n_best best words of every capture (sr_recognize_nbest_batch): the same dict with
        nbest NBEST_DTYPE [B, n_best] and n_matched uint32 [B].  rescore=True (sr_recognize_rescored_batch): also rescored
        NBEST_DTYPE [B, n_best] and n_rescored uint32 [B], the second pass of every list (rescore_nbest)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        buf_len = S if buf_len is None else buf_len
        K = self.n_templates
        res = np.zeros(B, dtype=RESULT_DTYPE)
        sc = np.zeros((B, K), dtype=np.uint32) if want_scores else None
        mf = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16) if want_mfcc else None
        vd = np.zeros(B, dtype=VAD_DTYPE) if want_vad else None
        nb = np.zeros((B, max(n_best, 0)), dtype=NBEST_DTYPE)
        nm = np.zeros(B, dtype=np.uint32)
        if rescore:
            rs = np.zeros((B, max(n_best, 0)), dtype=NBEST_DTYPE)
            nr = np.zeros(B, dtype=np.uint32)
            self._check(self.L.sr_recognize_rescored_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(buf_len), C.c_uint32(B),
                                                           C.c_uint32(n_best), _vp(nb), _vp(nm), _vp(rs), _vp(nr), _vp(res),
                                                           _vp(sc), _vp(mf), _vp(vd)))
            return dict(results=res, scores=sc, mfcc=mf, vad=vd, nbest=nb, n_matched=nm, rescored=rs, n_rescored=nr)
        self._check(self.L.sr_recognize_nbest_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(buf_len), C.c_uint32(B),
                                                    C.c_uint32(n_best), _vp(nb), _vp(nm), _vp(res), _vp(sc), _vp(mf), _vp(vd)))
        return dict(results=res, scores=sc, mfcc=mf, vad=vd, nbest=nb, n_matched=nm)

    # ---- host-buffer API --------------------------------------------------------------------------
    def recognize(self, pcm, want_scores=True, want_mfcc=True, want_vad=True, buf_len=None):
        """pcm uint16 [B, S] on the host.  Returns dict(results, scores, mfcc, vad) of numpy arrays."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        buf_len = S if buf_len is None else buf_len
        K = self.n_templates
        res = np.zeros(B, dtype=RESULT_DTYPE)
        sc = np.zeros((B, K), dtype=np.uint32) if want_scores else None
        mf = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16) if want_mfcc else None
        vd = np.zeros(B, dtype=VAD_DTYPE) if want_vad else None
        self._check(self.L.sr_recognize_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(buf_len), C.c_uint32(B),
                                              _vp(res), _vp(sc), _vp(mf), _vp(vd)))
        return dict(results=res, scores=sc, mfcc=mf, vad=vd)

    def recognize_packed12(self, packed, buf_len, want_scores=True, want_mfcc=True, want_vad=True):
        """packed uint8 [B, row_bytes]: 12-bit codes, two samples in three bytes (pack12()); sr_recognize_batch_packed12."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        B, rb = packed.shape
        K = self.n_templates
        res = np.zeros(B, dtype=RESULT_DTYPE)
        sc = np.zeros((B, K), dtype=np.uint32) if want_scores else None
        mf = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16) if want_mfcc else None
        vd = np.zeros(B, dtype=VAD_DTYPE) if want_vad else None
        self._check(self.L.sr_recognize_batch_packed12(self.h, _vp(packed), C.c_uint64(rb), C.c_uint32(buf_len), C.c_uint32(B),
                                                       _vp(res), _vp(sc), _vp(mf), _vp(vd)))
        return dict(results=res, scores=sc, mfcc=mf, vad=vd)

    def recognize_segments(self, pcm):
        """All VAD segments (extension of main.c:268).  Returns (results [max_seg, B], scores [max_seg, B, K], vad [B])."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        ms, K = self.cfg.max_seg, self.n_templates
        res = np.zeros((ms, B), dtype=RESULT_DTYPE)
        sc = np.zeros((ms, B, K), dtype=np.uint32)
        vd = np.zeros(B, dtype=VAD_DTYPE)
        self._check(self.L.sr_recognize_segments_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B),
                                                       _vp(res), _vp(sc), _vp(vd)))
        return res, sc, vd

    def segment_stream(self, pcm, lengths=None, atap=None, max_segs=None):
        """Stream VAD of recordings of any length (sr_recognize_stream without recognition): pcm uint16 [B, S],
        lengths [B] (None: S each), atap (None: noise_atap on each head, else an ATAP_DTYPE array [B]).
        Returns dict(segs [n] STREAM_SEG_DTYPE, seg_offsets [B+1], total); n = min(total, max_segs)."""
        return self.recognize_stream(pcm, lengths, atap, max_segs, recognize=False)

    def recognize_stream(self, pcm, lengths=None, atap=None, max_segs=None, want_scores=True, want_mfcc=True,
                         recognize=True, n_best=None):
        """Every segment of every recording recognised (sr_recognize_stream).  max_segs None: a first call counts the
        segments.  Returns dict(segs, seg_offsets, total, results, scores, mfcc) of numpy arrays, the
        per-segment outputs n = min(total, max_segs) long.  n_best (with recognize): sr_recognize_stream_nbest, the dict
        also holds nbest NBEST_DTYPE [n, n_best] and n_matched [n]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
        at = None if atap is None else np.ascontiguousarray(atap, dtype=ATAP_DTYPE)
        if max_segs is None:
            max_segs = int(self.recognize_stream(pcm, ln, at, 0, recognize=False)["total"])
        K = self.n_templates if recognize else 0
        segs = np.zeros(max_segs, dtype=STREAM_SEG_DTYPE)
        off = np.zeros(B + 1, dtype=np.uint32)
        res = np.zeros(max_segs, dtype=RESULT_DTYPE) if recognize else None
        sc = np.zeros((max_segs, K), dtype=np.uint32) if recognize and want_scores else None
        mf = np.zeros((max_segs, self.max_frames, self.n_coef), dtype=np.int16) if recognize and want_mfcc else None
        total = C.c_uint32(0)
        head = (self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), _vp(ln), C.c_uint32(B), _vp(at), C.c_uint32(max_segs),
                _vp(segs), _vp(off))
        cut = (lambda x: None if x is None else x[:min(total.value, max_segs)])
        if n_best is None or not recognize:
            self._check(self.L.sr_recognize_stream(*head, _vp(res), _vp(sc), _vp(mf), C.byref(total)))
            extra = {}
        else:
            nb = np.zeros((max_segs, max(n_best, 0)), dtype=NBEST_DTYPE)
            nm = np.zeros(max_segs, dtype=np.uint32)
            self._check(self.L.sr_recognize_stream_nbest(*head, C.c_uint32(n_best), _vp(nb), _vp(nm), _vp(res), _vp(sc),
                                                         _vp(mf), C.byref(total)))
            extra = dict(nbest=cut(nb), n_matched=cut(nm))
        return dict(segs=cut(segs), seg_offsets=off, total=total.value, results=cut(res), scores=cut(sc), mfcc=cut(mf),
                    **extra)

    def vad(self, pcm, buf_len=None):
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        vd = np.zeros(B, dtype=VAD_DTYPE)
        self._check(self.L.sr_vad_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S if buf_len is None else buf_len),
                                        C.c_uint32(B), _vp(vd)))
        return vd

    def vad_debug_masks(self, pcm, buf_len=None):
        """sr_vad_debug_masks (diagnostics): the VAD records of vad() and the per-frame "loud" bits (VAD.C:164) the kernel
        based them on, masks uint64 [B, 16]: bit k of word r = frame 63 * r + k (unpack_vad_masks).  A capture's words
        stay zero past the round in which its max_seg-th segment closed, and captures of more than 16 * 63 = 1 008 frames
        are outside what the diagnostic holds."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        vd = np.zeros(B, dtype=VAD_DTYPE)
        masks = np.zeros((B, VAD_MASK_WORDS), dtype=np.uint64)
        self._check(self.L.sr_vad_debug_masks(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S if buf_len is None else buf_len),
                                              C.c_uint32(B), _vp(vd), _vp(masks)))
        return vd, masks

    def mfcc(self, pcm, start, end, mid):
        """get_mfcc of segment [start[b], end[b]) of row b with mid value mid[b]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16)
        n = np.zeros(B, dtype=np.uint32)
        self._check(self.L.sr_mfcc_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start),
                                         _vp(end), _vp(mid), _vp(out), _vp(n)))
        return n, out

    def mfcc_status(self, pcm, start, end, mid):
        """like mfcc(), with per-record failure instead of a batch error (sr_mfcc_batch_status): returns
        (frm_num, mfcc, status); a bad record has frm_num 0, an all-zero MFCC record and status != 0."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16)
        n = np.zeros(B, dtype=np.uint32)
        st = np.zeros(B, dtype=np.uint32)
        self._check(self.L.sr_mfcc_batch_status(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start),
                                                _vp(end), _vp(mid), _vp(out), _vp(n), _vp(st)))
        return n, out, st

    def frame_feature_width(self, kind):
        """sr_frame_feature_width: u32 words per frame of a feature kind (0 for an unknown kind)"""
        self.L.sr_frame_feature_width.restype = C.c_uint32
        return int(self.L.sr_frame_feature_width(self.h, C.c_int(kind)))

    def frame_features(self, pcm, start, end, mid, kind, want_mfcc=False):
        """Per-frame intermediate values of get_mfcc for segment [start[b], end[b]) of row b (sr_frame_features_batch):
        kind FEAT_FFT / FEAT_MAG (uint32 [B, max_frames, nfft/2]) or FEAT_MEL / FEAT_LOGMEL ([B, max_frames, n_mel]), rows
        >= frm_num zero.  Returns (feat, frm_num, status), and the MFCC rows of the same launch as a fourth item when
        want_mfcc.  Failed records as in mfcc_status()."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        width = self.frame_feature_width(kind)
        feat = np.zeros((B, self.max_frames, max(width, 1)), dtype=np.uint32)
        mf = np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16) if want_mfcc else None
        n = np.zeros(B, dtype=np.uint32)
        st = np.zeros(B, dtype=np.uint32)
        self._check(self.L.sr_frame_features_batch(self.h, C.c_int(kind), _vp(pcm), C.c_uint64(S), C.c_uint32(S),
                                                   C.c_uint32(B), _vp(start), _vp(end), _vp(mid), _vp(feat), _vp(mf),
                                                   _vp(n), _vp(st)))
        return (feat, n, st, mf) if want_mfcc else (feat, n, st)

    def dtw(self, in_mfcc, in_frames):
        """in_mfcc int16 [B, max_frames, 12] against the template store -> (scores [B,K], results [B])."""
        in_mfcc = np.ascontiguousarray(in_mfcc, dtype=np.int16)
        assert in_mfcc.shape[1:] == (self.max_frames, self.n_coef)
        in_frames = np.ascontiguousarray(in_frames, dtype=np.uint32)
        B = in_mfcc.shape[0]
        sc = np.zeros((B, self.n_templates), dtype=np.uint32)
        res = np.zeros(B, dtype=RESULT_DTYPE)
        self._check(self.L.sr_dtw_batch(self.h, _vp(in_mfcc), _vp(in_frames), C.c_uint32(B), _vp(sc), _vp(res)))
        return sc, res

    def dtw_dp(self, in_mfcc, in_frames):
        """OPT-IN non-reference scorer: full-DP DTW scores [B, K] (see sr_dtw_dp_batch)."""
        in_mfcc = np.ascontiguousarray(in_mfcc, dtype=np.int16)
        assert in_mfcc.shape[1:] == (self.max_frames, self.n_coef)
        in_frames = np.ascontiguousarray(in_frames, dtype=np.uint32)
        B = in_mfcc.shape[0]
        sc = np.zeros((B, self.n_templates), dtype=np.uint32)
        self._check(self.L.sr_dtw_dp_batch(self.h, _vp(in_mfcc), _vp(in_frames), C.c_uint32(B), _vp(sc)))
        return sc

    def set_dp_lanes(self, lanes=0):
        """lanes per pair of the opt-in full-DP scorer: 0 default (8), 4 / 8 / 16 band kernel, 1 = one wave per pair"""
        self._check(self.L.sr_set_dp_lanes(self.h, C.c_uint32(lanes)))

    def set_small_launch(self, mode=0):
        """Small-launch forms of the kernels (four waves per capture in VAD, 4-frame workgroups in the frame kernel, one
        workgroup per DTW pair + in-kernel slot scan, four lanes per DTW pair for mid-sized launches, pinned host staging):
        0 automatic by launch size, 1 never, 2 always (DTW: one workgroup per pair whenever the in x mdl rectangle fits a
        workgroup's LDS), 3 the four-lanes-per-pair DTW form whenever the sequences fit.  Same results in every mode."""
        self._check(self.L.sr_set_small_launch(self.h, C.c_int(mode)))

    def dtw_dp_dev(self, mfcc, scores, in_frames=None, vad=None, stream=None):
        """OPT-IN non-reference scorer on device tensors: mfcc int16 [B, max_frames, 12], frame counts from in_frames
        (int32 [B]) or vad records; scores int32 [B, K].  Asynchronous on `stream`."""
        import torch
        B = mfcc.shape[0]
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_dtw_dp_batch_dev(self.h, _vp(mfcc), _vp(in_frames), _vp(vad), C.c_uint32(B), _vp(scores),
                                               C.c_void_p(stream)))
        return scores

    def spot_windows(self, win_frames=0):
        """windows per row of a spotting call with this engine's max_frames (sr_spot_geometry's out[0])"""
        return 1 if win_frames == 0 else -(-self.max_frames // win_frames)

    def spot(self, mfcc, frames, win_frames=0):
        """OPT-IN word spotter (sr_spot_dp_batch): where inside each feature row every template matches best.  mfcc int16
        [n_rows, max_frames, 12], frames uint32 [n_rows]; win_frames 0 = one window per row.  Returns (hits SPOT_DTYPE
        [n_rows, n_win, K], scores uint32 [n_rows, n_win, K] = the dis fields, the layout nbest() takes)."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        shape = (n, self.spot_windows(win_frames), self.n_templates)
        hits, sc = np.zeros(shape, dtype=SPOT_DTYPE), np.zeros(shape, dtype=np.uint32)
        self._check(self.L.sr_spot_dp_batch(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), C.c_uint32(win_frames),
                                            _vp(hits), _vp(sc)))
        return hits, sc

    def spot_dev(self, mfcc, frames, hits, scores=None, win_frames=0, frames_stride=1, stream=None):
        """sr_spot_dp_batch_dev on device tensors: mfcc int16 [n_rows, max_frames, 12]; frames as for rescore_nbest_dev (the
        first row's count, the next one frames_stride 32-bit words further on: 12 for vad[:, 9]); hits int32 [n_rows, n_win,
        K, 4]; scores (optional) int32 [n_rows, n_win, K].  Asynchronous on `stream`; returns hits."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and hits.is_contiguous()
        n = mfcc.shape[0]
        assert hits.numel() == n * self.spot_windows(win_frames) * self.n_templates * 4
        assert scores is None or (scores.is_contiguous() and scores.numel() * 4 == hits.numel())
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_spot_dp_batch_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                C.c_uint32(win_frames), _vp(hits), _vp(scores), C.c_void_p(stream)))
        return hits

    def spot_pcm(self, pcm, start, end, mid, win_frames=0):
        """sr_spot_batch, the host whole path: mfcc_status() of segment [start[b], end[b]) of row b, then spot() over those
        rows.  Returns dict(hits, scores, mfcc, frm_num, status); a failed record has no hits."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        shape = (B, self.spot_windows(win_frames), self.n_templates)
        out = dict(hits=np.zeros(shape, dtype=SPOT_DTYPE), scores=np.zeros(shape, dtype=np.uint32),
                   mfcc=np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16), frm_num=np.zeros(B, dtype=np.uint32),
                   status=np.zeros(B, dtype=np.uint32))
        self._check(self.L.sr_spot_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start), _vp(end),
                                         _vp(mid), C.c_uint32(win_frames), _vp(out["hits"]), _vp(out["scores"]),
                                         _vp(out["mfcc"]), _vp(out["frm_num"]), _vp(out["status"])))
        return out

    # ---- connected-word decoding ----------------------------------------------------------------------------
    @staticmethod
    def _skip(skip_cost):
        return DIS_ERR if skip_cost is None else int(skip_cost)

    def decode_words(self, mfcc, frames, max_words=8, n_words=0, skip_cost=None, word_cost=0):
        """OPT-IN connected-word decoder (sr_decode_words_dp): which sequence of words each feature row contains, by
        level-building DTW over the template store.  mfcc int16 [n_rows, max_frames, 12], frames uint32 [n_rows]; n_words 0 =
        the cheapest count of 1..max_words; skip_cost None = every frame belongs to a word.  Returns (rec CHAIN_REC_DTYPE
        [n_rows], words CHAIN_WORD_DTYPE [n_rows, max_words] in spoken order, level_cost uint32 [n_rows, max_words])."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, max_words), dtype=CHAIN_WORD_DTYPE)
        lc = np.zeros((n, max_words), dtype=np.uint32)
        self._check(self.L.sr_decode_words_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), C.c_uint32(max_words),
                                              C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(rec),
                                              _vp(words), _vp(lc)))
        return rec, words, lc

    def decode_words_dev(self, mfcc, frames, rec, words, level_cost=None, max_words=8, n_words=0, skip_cost=None, word_cost=0,
                         frames_stride=1, stream=None):
        """sr_decode_words_dp_dev on device tensors: mfcc int16 [n_rows, max_frames, 12]; frames as for spot_dev; rec int32
        [n_rows, 4]; words int32 [n_rows, max_words, 8]; level_cost (optional) int32 [n_rows, max_words].  Asynchronous on
        `stream`; returns (rec, words, level_cost)."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and words.numel() == n * max_words * 8
        assert level_cost is None or (level_cost.is_contiguous() and level_cost.numel() == n * max_words)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_decode_words_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                  C.c_uint32(max_words), C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)),
                                                  C.c_uint32(word_cost), _vp(rec), _vp(words), _vp(level_cost), C.c_void_p(stream)))
        return rec, words, level_cost

    def decode_words_pcm(self, pcm, start, end, mid, max_words=8, n_words=0, skip_cost=None, word_cost=0):
        """sr_decode_words_batch, the host whole path: mfcc_status() of segment [start[b], end[b]) of row b, then
        decode_words() over those rows.  Returns dict(rec, words, level_cost, mfcc, frm_num, status); a failed record has
        no parse."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = dict(rec=np.zeros(B, dtype=CHAIN_REC_DTYPE), words=np.zeros((B, max_words), dtype=CHAIN_WORD_DTYPE),
                   level_cost=np.zeros((B, max_words), dtype=np.uint32),
                   mfcc=np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16), frm_num=np.zeros(B, dtype=np.uint32),
                   status=np.zeros(B, dtype=np.uint32))
        self._check(self.L.sr_decode_words_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start), _vp(end),
                                                 _vp(mid), C.c_uint32(max_words), C.c_uint32(n_words),
                                                 C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(out["rec"]),
                                                 _vp(out["words"]), _vp(out["level_cost"]), _vp(out["mfcc"]), _vp(out["frm_num"]),
                                                 _vp(out["status"])))
        return out

    # ---- one-pass connected-word decoding ---------------------------------------------------------------------
    def decode_onepass(self, mfcc, frames, words_cap=64, skip_cost=None, word_cost=0, frames_cap=0):
        """OPT-IN one-pass connected-word decoder (sr_decode_onepass_dp): decode_words() without a word cap and at a cost
        that does not grow with the word count -- one prefix-cost array over all word counts.  mfcc int16 [n_rows, max_frames,
        12], frames uint32 [n_rows]; frames_cap = a bound on every row's frames (0 = max_frames; fewer blocks are launched for a
        smaller one); skip_cost None = every frame belongs to a word.  Returns (rec CHAIN_REC_DTYPE [n_rows], words
        CHAIN_WORD_DTYPE [n_rows, words_cap] in spoken order); a row with more than words_cap words has status CH_TRUNCATED,
        its true n_words and its first words_cap words."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, max(words_cap, 1)), dtype=CHAIN_WORD_DTYPE)
        self._check(self.L.sr_decode_onepass_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), C.c_uint32(frames_cap),
                                                C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost),
                                                _vp(rec), _vp(words)))
        return rec, words

    def decode_onepass_dev(self, mfcc, frames, rec, words, words_cap=64, skip_cost=None, word_cost=0, frames_cap=0, frames_stride=1,
                           stream=None):
        """sr_decode_onepass_dp_dev on device tensors: mfcc int16 [n_rows, max_frames, 12]; frames as for spot_dev; rec int32
        [n_rows, 4]; words int32 [n_rows, words_cap, 8].  Asynchronous on `stream`; returns (rec, words)."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and words.numel() == n * words_cap * 8
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_decode_onepass_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                    C.c_uint32(frames_cap), C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)),
                                                    C.c_uint32(word_cost), _vp(rec), _vp(words), C.c_void_p(stream)))
        return rec, words

    def decode_onepass_pcm(self, pcm, start, end, mid, words_cap=64, skip_cost=None, word_cost=0):
        """sr_decode_onepass_batch, the host whole path: mfcc_status() of segment [start[b], end[b]) of row b, then
        decode_onepass() over those rows.  Returns dict(rec, words, mfcc, frm_num, status); a failed record has no parse."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = dict(rec=np.zeros(B, dtype=CHAIN_REC_DTYPE), words=np.zeros((B, max(words_cap, 1)), dtype=CHAIN_WORD_DTYPE),
                   mfcc=np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16), frm_num=np.zeros(B, dtype=np.uint32),
                   status=np.zeros(B, dtype=np.uint32))
        self._check(self.L.sr_decode_onepass_batch(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start), _vp(end),
                                                   _vp(mid), C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)),
                                                   C.c_uint32(word_cost), _vp(out["rec"]), _vp(out["words"]), _vp(out["mfcc"]),
                                                   _vp(out["frm_num"]), _vp(out["status"])))
        return out

    # ---- word alternatives ----------------------------------------------------------------------------------
    def score_word_spans(self, mfcc, frames, words, mode=0):
        """OPT-IN span scorer (sr_score_word_spans): the best path of EVERY template over fixed spans of frames, start and end
        pinned.  mfcc int16 [n_rows, max_frames, 12], frames uint32 [n_rows], words CHAIN_WORD_DTYPE [n_rows, words_per_row]
        (any decoder's word rows, or spans of the caller's making: only start and end are read; all ones = no span); mode
        SPAN_ACC = path costs, SPAN_DIS = cost / (L + M).  Returns scores uint32 [n_rows, words_per_row, K], DIS_ERR where
        the slot has no path over the span: the layout nbest() takes."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=CHAIN_WORD_DTYPE)
        n = mfcc.shape[0]
        assert len(frames) == n and words.ndim == 2 and words.shape[0] == n
        sc = np.zeros((n, words.shape[1], self.n_templates), dtype=np.uint32)
        self._check(self.L.sr_score_word_spans(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), C.c_uint32(words.shape[1]),
                                               _vp(words), C.c_uint32(mode), _vp(sc)))
        return sc

    def score_word_spans_dev(self, mfcc, frames, words, scores, mode=0, frames_stride=1, stream=None):
        """sr_score_word_spans_dev on device tensors: mfcc int16 [n_rows, max_frames, 12]; frames as for spot_dev; words int32
        [n_rows, words_per_row, 8] (decode_words_dev's, decode_grammar_dev's or a session's word rows as they are); scores
        int32 [n_rows, words_per_row, K].  Asynchronous on `stream`; returns scores."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and words.is_contiguous() and scores.is_contiguous()
        n = mfcc.shape[0]
        wpr = words.numel() // (8 * max(n, 1))
        assert words.numel() == n * wpr * 8 and scores.numel() == n * wpr * self.n_templates
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_score_word_spans_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                   C.c_uint32(wpr), _vp(words), C.c_uint32(mode), _vp(scores), C.c_void_p(stream)))
        return scores

    def decode_words_alts(self, mfcc, frames, max_words=8, n_best=4, mode=0, n_words=0, skip_cost=None, word_cost=0, want_scores=False):
        """decode_words() with alternatives (sr_decode_words_alts): per decoded word the n_best best words of the store over
        that word's frames, under the engine's word map.  Returns decode_words()'s (rec, words, level_cost) -- the same
        bytes -- plus alts NBEST_DTYPE [n_rows, max_words, n_best] and n_matched uint32 [n_rows, max_words], and with
        want_scores the span scores uint32 [n_rows, max_words, K].  In mode SPAN_ACC entry 0 of a word is the decoded slot
        at its `acc`; alts[.., 1]["dis"] - alts[.., 0]["dis"] is the word's margin over the runner-up."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, max_words), dtype=CHAIN_WORD_DTYPE)
        lc = np.zeros((n, max_words), dtype=np.uint32)
        alts, nm = np.zeros((n, max_words, max(n_best, 0)), dtype=NBEST_DTYPE), np.zeros((n, max_words), dtype=np.uint32)
        sc = np.zeros((n, max_words, self.n_templates), dtype=np.uint32) if want_scores else None
        self._check(self.L.sr_decode_words_alts(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), C.c_uint32(max_words),
                                                C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(rec),
                                                _vp(words), _vp(lc), C.c_uint32(n_best), C.c_uint32(mode), _vp(alts), _vp(nm), _vp(sc)))
        return (rec, words, lc, alts, nm, sc) if want_scores else (rec, words, lc, alts, nm)

    def decode_words_alts_dev(self, mfcc, frames, rec, words, alts, level_cost=None, n_matched=None, span_scores=None, max_words=8,
                              mode=0, n_words=0, skip_cost=None, word_cost=0, frames_stride=1, stream=None):
        """sr_decode_words_alts_dev on device tensors: decode_words_dev()'s tensors plus alts int32 [n_rows, max_words, n_best,
        4], n_matched (optional) int32 [n_rows, max_words] and span_scores (optional) int32 [n_rows, max_words, K].  One
        asynchronous operation on `stream`; returns (rec, words, level_cost, alts, n_matched, span_scores)."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous() and alts.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and words.numel() == n * max_words * 8
        assert level_cost is None or (level_cost.is_contiguous() and level_cost.numel() == n * max_words)
        n_best = alts.numel() // (4 * max(n * max_words, 1))
        assert alts.numel() == n * max_words * n_best * 4
        assert n_matched is None or (n_matched.is_contiguous() and n_matched.numel() == n * max_words)
        assert span_scores is None or (span_scores.is_contiguous() and span_scores.numel() == n * max_words * self.n_templates)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_decode_words_alts_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                    C.c_uint32(max_words), C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)),
                                                    C.c_uint32(word_cost), _vp(rec), _vp(words), _vp(level_cost), C.c_uint32(n_best),
                                                    C.c_uint32(mode), _vp(alts), _vp(n_matched), _vp(span_scores), C.c_void_p(stream)))
        return rec, words, level_cost, alts, n_matched, span_scores

    # ---- grammar-constrained decoding ---------------------------------------------------------------------
    def grammar(self, n_states, arcs, final, arc_cost=None, final_cost=None):
        """sr_grammar_create[_weighted]: a Grammar compiled against the current store and word map.  States 0..n_states - 1,
        state 0 the start; arcs = (from, to, word label) triples; final[s] != 0 flags the final states.  arc_cost [n_arcs] and
        final_cost [n_states] (each None = all 0, at most 2^24, final_cost 0 on a state that is not final) are added to the
        acoustic cost of a parse: the weighted grammars of the header.  The grammar_* helpers return exactly these arguments:
        eng.grammar(*grammar_sequence([...])), eng.grammar(*grammar_bigram(...))."""
        return Grammar(self, n_states, arcs, final, arc_cost, final_cost)

    def decode_grammar(self, gram, mfcc, frames, max_words=8, n_words=0, skip_cost=None, word_cost=0):
        """decode_words() under a Grammar (sr_decode_grammar_dp): the cheapest parse among the word sequences the grammar
        accepts; the word rows' `reserved` holds the grammar state after each word."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, max_words), dtype=CHAIN_WORD_DTYPE)
        lc = np.zeros((n, max_words), dtype=np.uint32)
        self._check(self.L.sr_decode_grammar_dp(self.h, gram.g, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n),
                                                C.c_uint32(max_words), C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)),
                                                C.c_uint32(word_cost), _vp(rec), _vp(words), _vp(lc)))
        return rec, words, lc

    def decode_grammar_dev(self, gram, mfcc, frames, rec, words, level_cost=None, max_words=8, n_words=0, skip_cost=None,
                           word_cost=0, frames_stride=1, stream=None):
        """decode_words_dev() under a Grammar (sr_decode_grammar_dp_dev): the same tensors, asynchronous on `stream`."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and words.numel() == n * max_words * 8
        assert level_cost is None or (level_cost.is_contiguous() and level_cost.numel() == n * max_words)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_decode_grammar_dp_dev(self.h, gram.g, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                    C.c_uint32(max_words), C.c_uint32(n_words), C.c_uint32(self._skip(skip_cost)),
                                                    C.c_uint32(word_cost), _vp(rec), _vp(words), _vp(level_cost), C.c_void_p(stream)))
        return rec, words, level_cost

    def decode_grammar_pcm(self, gram, pcm, start, end, mid, max_words=8, n_words=0, skip_cost=None, word_cost=0):
        """decode_words_pcm() under a Grammar (sr_decode_grammar_batch): the same dict."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = dict(rec=np.zeros(B, dtype=CHAIN_REC_DTYPE), words=np.zeros((B, max_words), dtype=CHAIN_WORD_DTYPE),
                   level_cost=np.zeros((B, max_words), dtype=np.uint32),
                   mfcc=np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16), frm_num=np.zeros(B, dtype=np.uint32),
                   status=np.zeros(B, dtype=np.uint32))
        self._check(self.L.sr_decode_grammar_batch(self.h, gram.g, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start),
                                                   _vp(end), _vp(mid), C.c_uint32(max_words), C.c_uint32(n_words),
                                                   C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(out["rec"]),
                                                   _vp(out["words"]), _vp(out["level_cost"]), _vp(out["mfcc"]), _vp(out["frm_num"]),
                                                   _vp(out["status"])))
        return out

    # ---- one-pass grammar decoding ------------------------------------------------------------------------------
    def decode_onepass_grammar(self, gram, mfcc, frames, words_cap=64, skip_cost=None, word_cost=0, frames_cap=0):
        """OPT-IN one-pass grammar decoder (sr_decode_onepass_grammar_dp): decode_onepass() under a Grammar, weighted or not --
        the cheapest parse among the word sequences the grammar accepts, without a word cap.  Arguments and returns as
        decode_onepass(); the word rows' `reserved` holds the grammar state after each word."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, max(words_cap, 1)), dtype=CHAIN_WORD_DTYPE)
        self._check(self.L.sr_decode_onepass_grammar_dp(self.h, gram.g, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n),
                                                        C.c_uint32(frames_cap), C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)),
                                                        C.c_uint32(word_cost), _vp(rec), _vp(words)))
        return rec, words

    def decode_onepass_grammar_dev(self, gram, mfcc, frames, rec, words, words_cap=64, skip_cost=None, word_cost=0, frames_cap=0,
                                   frames_stride=1, stream=None):
        """decode_onepass_dev() under a Grammar (sr_decode_onepass_grammar_dp_dev): the same tensors, asynchronous on `stream`."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and words.numel() == n * words_cap * 8
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_decode_onepass_grammar_dp_dev(self.h, gram.g, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                            C.c_uint32(frames_cap), C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)),
                                                            C.c_uint32(word_cost), _vp(rec), _vp(words), C.c_void_p(stream)))
        return rec, words

    def decode_onepass_grammar_pcm(self, gram, pcm, start, end, mid, words_cap=64, skip_cost=None, word_cost=0):
        """decode_onepass_pcm() under a Grammar (sr_decode_onepass_grammar_batch): the same dict."""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mid = np.ascontiguousarray(mid, dtype=np.uint32)
        out = dict(rec=np.zeros(B, dtype=CHAIN_REC_DTYPE), words=np.zeros((B, max(words_cap, 1)), dtype=CHAIN_WORD_DTYPE),
                   mfcc=np.zeros((B, self.max_frames, self.n_coef), dtype=np.int16), frm_num=np.zeros(B, dtype=np.uint32),
                   status=np.zeros(B, dtype=np.uint32))
        self._check(self.L.sr_decode_onepass_grammar_batch(self.h, gram.g, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(start),
                                                           _vp(end), _vp(mid), C.c_uint32(words_cap), C.c_uint32(self._skip(skip_cost)),
                                                           C.c_uint32(word_cost), _vp(out["rec"]), _vp(out["words"]), _vp(out["mfcc"]),
                                                           _vp(out["frm_num"]), _vp(out["status"])))
        return out

    def decode_live(self, n_channels, chunk_max, utt_frames, max_words=8, n_words=0, skip_cost=None, word_cost=0, mid=None):
        """sr_decode_live_open: a DecodeSession of n_channels channels of at most utt_frames frames each.  mid None: a feature
        session (chunk_max in frames); mid uint32 [n_channels]: a PCM session (chunk_max in samples)."""
        return DecodeSession(self, n_channels, chunk_max, utt_frames, max_words, n_words, skip_cost, word_cost, mid)

    def decode_grammar_live(self, gram, n_channels, chunk_max, utt_frames, max_words=8, n_words=0, skip_cost=None, word_cost=0,
                            mid=None):
        """sr_gram_live_open: a GrammarSession -- decode_live() under a Grammar, which sess.set_grammar() switches between
        recordings.  Close the session before the grammar."""
        return GrammarSession(self, gram, n_channels, chunk_max, utt_frames, max_words, n_words, skip_cost, word_cost, mid)

    def decode_onepass_live(self, n_channels, chunk_max, utt_frames, words_cap, tail=False, skip_cost=None, word_cost=0, mid=None):
        """sr_onepass_live_open: an OnePassSession -- decode_onepass() push by push, no word cap.  tail: a row holds the LAST
        words_cap words of the parse (OP_LIVE_TAIL) instead of the first.  mid as for decode_live."""
        return OnePassSession(self, n_channels, chunk_max, utt_frames, words_cap, tail, skip_cost, word_cost, mid)

    def decode_onepass_grammar_live(self, gram, n_channels, chunk_max, utt_frames, words_cap, tail=False, skip_cost=None, word_cost=0,
                                    mid=None):
        """sr_onepass_gram_live_open: an OnePassGrammarSession -- decode_onepass_grammar() push by push, no word cap; the
        session's set_grammar() switches the grammar between recordings.  tail and mid as for decode_onepass_live.  Close the
        session before the grammar."""
        return OnePassGrammarSession(self, gram, n_channels, chunk_max, utt_frames, words_cap, tail, skip_cost, word_cost, mid)

    # ---- full-DP alignment and word models from many examples -----------------------------------------
    def align(self, mfcc, frames, ref, ref_frames, ref_of_row=None, want_span=True):
        """OPT-IN (sr_dtw_dp_align): the optimal warping path of the full-DP scorer for every (row, reference) pair.  mfcc int16
        [n, max_frames, 12], frames uint32 [n]; ref int16 [n_ref, ref_rows, 12], ref_frames uint32 [n_ref]; ref_of_row uint32
        [n] or None (row r pairs with reference r).  Returns (rec ALIGN_DTYPE [n], span uint32 [n, max_frames] or None):
        span[r, x] = y_first | y_last << 16, 0xFFFFFFFF past the row's frames and for a pair that was not aligned."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        ref = np.ascontiguousarray(ref, dtype=np.int16)
        ref_frames = np.ascontiguousarray(ref_frames, dtype=np.uint32)
        n, n_ref = mfcc.shape[0], ref.shape[0]
        assert len(frames) == n and ref.shape[2] == N_COEF and len(ref_frames) == n_ref
        if ref_of_row is not None:
            ref_of_row = np.ascontiguousarray(ref_of_row, dtype=np.uint32)
            assert len(ref_of_row) == n
        rec = np.zeros(n, dtype=ALIGN_DTYPE)
        span = np.zeros((n, self.max_frames), dtype=np.uint32) if want_span else None
        self._check(self.L.sr_dtw_dp_align(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), _vp(ref), _vp(ref_frames),
                                           C.c_uint32(ref.shape[1]), C.c_uint32(n_ref), _vp(ref_of_row), _vp(rec), _vp(span)))
        return rec, span

    def align_dev(self, mfcc, frames, ref, ref_frames, rec, span=None, ref_of_row=None, frames_stride=1, stream=None):
        """sr_dtw_dp_align_dev on device tensors: mfcc int16 [n, max_frames, 12]; frames as for rescore_nbest_dev; ref int16
        [n_ref, ref_rows, 12], ref_frames int32 [n_ref]; rec int32 [n, 4]; span (optional) int32 [n, max_frames]; ref_of_row
        (optional) int32 [n].  Asynchronous on `stream`; returns rec."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and ref.is_contiguous() and rec.is_contiguous()
        n = mfcc.shape[0]
        assert rec.numel() == n * 4 and (span is None or (span.is_contiguous() and span.numel() == n * self.max_frames))
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_dtw_dp_align_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n), _vp(ref),
                                               _vp(ref_frames), C.c_uint32(ref.shape[1]), C.c_uint32(ref.shape[0]), _vp(ref_of_row),
                                               _vp(rec), _vp(span), C.c_void_p(stream)))
        return rec

    def train_models(self, mfcc, frames, ex_start, cen, cen_frames, n_iter=4):
        """OPT-IN (sr_train_models_dp): DTW barycentre averaging.  Model m is refined from the example rows
        [ex_start[m], ex_start[m + 1]) of mfcc int16 [E, max_frames, 12] (frames uint32 [E]), starting from cen int16
        [M, cen_rows, 12] with cen_frames uint32 [M].  Returns (centroids int16 [M, cen_rows, 12] -- with cen_frames the layout
        set_templates_dense takes --, stats TRAIN_STAT_DTYPE [n_iter, M])."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        ex_start = np.ascontiguousarray(ex_start, dtype=np.uint32)
        cen = np.ascontiguousarray(cen, dtype=np.int16)
        cen_frames = np.ascontiguousarray(cen_frames, dtype=np.uint32)
        M = cen.shape[0]
        assert cen.shape[2] == N_COEF and len(cen_frames) == M and len(ex_start) == M + 1 and len(frames) == mfcc.shape[0]
        assert int(ex_start[-1]) <= mfcc.shape[0]
        out = np.zeros_like(cen)
        stats = np.zeros((n_iter, M), dtype=TRAIN_STAT_DTYPE)
        self._check(self.L.sr_train_models_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), _vp(ex_start), C.c_uint32(M), _vp(cen),
                                              _vp(cen_frames), C.c_uint32(cen.shape[1]), C.c_uint32(n_iter), _vp(out), _vp(stats)))
        return out, stats

    def train_models_dev(self, mfcc, frames, ex_start, cen_in, cen_frames, cen_out, n_iter=4, stats=None, frames_stride=1, stream=None):
        """sr_train_models_dp_dev on device tensors (ex_start: a HOST sequence of M + 1 counts): cen_in / cen_out int16
        [M, cen_rows, 12], cen_frames int32 [M], stats (optional) int32 [n_iter, M, 4].  One asynchronous operation on `stream`;
        returns cen_out."""
        import torch
        ex_start = np.ascontiguousarray(ex_start, dtype=np.uint32)
        M = cen_in.shape[0]
        assert mfcc.is_cuda and mfcc.is_contiguous() and cen_in.is_contiguous() and cen_out.is_contiguous()
        assert len(ex_start) == M + 1 and int(ex_start[-1]) <= mfcc.shape[0] and cen_out.shape == cen_in.shape
        assert stats is None or (stats.is_contiguous() and stats.numel() * stats.element_size() == n_iter * M * 16)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_train_models_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), _vp(ex_start), C.c_uint32(M),
                                                  _vp(cen_in), _vp(cen_frames), C.c_uint32(cen_in.shape[1]), C.c_uint32(n_iter),
                                                  _vp(cen_out), _vp(stats), C.c_void_p(stream)))
        return cen_out

    def train_words(self, mfcc, frames, labels, n_iter=4, init=None):
        """Word models from labelled examples: the rows are grouped by label (ascending label, rows of a word in their order),
        each word starts from its first example -- or from init = (centroids int16 [M, rows, 12], frames [M]) in ascending
        label order -- and train_models refines it.  Returns (centroids int16 [M, rows, 12], frames uint32 [M], word_ids
        uint32 [M]): set_templates_dense(centroids, frames) and set_word_map(word_ids) make them the store."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.minimum(np.ascontiguousarray(frames, dtype=np.uint32), self.max_frames)
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        assert len(labels) == len(frames) == mfcc.shape[0]
        word_ids, counts = np.unique(labels, return_counts=True)
        order = np.argsort(labels, kind="stable")
        ex_start = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
        if init is None:
            first = order[ex_start[:-1]]
            cen_frames = frames[first]
            cen = np.zeros((len(word_ids), max(int(cen_frames.max()), 1) + 1, N_COEF), np.int16)  # (one row of slack, as a store has)
            for m, e in enumerate(first):
                cen[m, :cen_frames[m]] = mfcc[e, :cen_frames[m]]
        else:
            cen, cen_frames = np.ascontiguousarray(init[0], dtype=np.int16), np.ascontiguousarray(init[1], dtype=np.uint32)
            assert cen.shape[0] == len(word_ids) == len(cen_frames)
        out, _ = self.train_models(mfcc[order], frames[order], ex_start, cen, cen_frames, n_iter)
        return out, cen_frames.copy(), word_ids.astype(np.uint32)

    # ---- word models: clustering a word's examples into several templates ----------------------------------
    def _cluster_in(self, mfcc, frames, word_start, mdl_start, cen, cen_frames):
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        word_start = np.ascontiguousarray(word_start, dtype=np.uint32)
        mdl_start = np.ascontiguousarray(mdl_start, dtype=np.uint32)
        cen = np.ascontiguousarray(cen, dtype=np.int16)
        cen_frames = np.ascontiguousarray(cen_frames, dtype=np.uint32)
        assert len(word_start) == len(mdl_start) >= 2 and cen.shape[2] == N_COEF and len(cen_frames) == cen.shape[0]
        assert int(word_start[-1]) <= mfcc.shape[0] == len(frames) and int(mdl_start[-1]) <= cen.shape[0]
        return mfcc, frames, word_start, mdl_start, cen, cen_frames

    def cluster_assign(self, mfcc, frames, word_start, mdl_start, cen, cen_frames, want_scores=True):
        """OPT-IN (sr_cluster_assign): which model of its word every example is closest to under the full-DP aligner's dis.
        Word w owns the rows [word_start[w], word_start[w + 1]) of mfcc int16 [E, max_frames, 12] and the models
        [mdl_start[w], mdl_start[w + 1]) of cen int16 [M, cen_rows, 12] (cen_frames uint32 [M]).  Returns (assign uint32 [E]
        -- a model index, CLUSTER_NONE where no model admits the example --, best uint32 [E], scores uint32 [E, 16] or None:
        column c = the word's model c, DIS_ERR past its model count)."""
        mfcc, frames, word_start, mdl_start, cen, cen_frames = self._cluster_in(mfcc, frames, word_start, mdl_start, cen, cen_frames)
        E = int(word_start[-1])
        assign, best = np.zeros(E, np.uint32), np.zeros(E, np.uint32)
        scores = np.zeros((E, CLUSTER_MAX), np.uint32) if want_scores else None
        self._check(self.L.sr_cluster_assign(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), _vp(word_start), _vp(mdl_start),
                                             C.c_uint32(len(word_start) - 1), _vp(cen), _vp(cen_frames), C.c_uint32(cen.shape[1]),
                                             _vp(assign), _vp(best), _vp(scores)))
        return assign, best, scores

    def cluster_assign_dev(self, mfcc, frames, word_start, mdl_start, cen, cen_frames, assign, best=None, scores=None, frames_stride=1,
                           stream=None):
        """sr_cluster_assign_dev on device tensors (word_start / mdl_start: HOST sequences of W + 1 counts): assign int32 [E],
        best (optional) int32 [E], scores (optional) int32 [E, 16].  One asynchronous operation on `stream`; returns assign."""
        import torch
        word_start = np.ascontiguousarray(word_start, dtype=np.uint32)
        mdl_start = np.ascontiguousarray(mdl_start, dtype=np.uint32)
        E = int(word_start[-1])
        assert mfcc.is_cuda and mfcc.is_contiguous() and cen.is_contiguous() and assign.is_contiguous() and assign.numel() == E
        assert len(word_start) == len(mdl_start) and E <= mfcc.shape[0] and int(mdl_start[-1]) <= cen.shape[0]
        assert best is None or (best.is_contiguous() and best.numel() == E)
        assert scores is None or (scores.is_contiguous() and scores.numel() == E * CLUSTER_MAX)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_cluster_assign_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), _vp(word_start), _vp(mdl_start),
                                                 C.c_uint32(len(word_start) - 1), _vp(cen), _vp(cen_frames), C.c_uint32(cen.shape[1]),
                                                 _vp(assign), _vp(best), _vp(scores), C.c_void_p(stream)))
        return assign

    def cluster_models(self, mfcc, frames, word_start, mdl_start, cen, cen_frames, n_iter=4):
        """OPT-IN (sr_cluster_models_dp): k-means under DTW.  Per iteration every example goes to the nearest model of its word
        (cluster_assign's rule) and every model is re-averaged from the examples it received (one train_models iteration).
        Returns (centroids int16 like cen, assign uint32 [E] of the last iteration, stats TRAIN_STAT_DTYPE [n_iter, M], iter
        CLUSTER_ITER_DTYPE [n_iter])."""
        mfcc, frames, word_start, mdl_start, cen, cen_frames = self._cluster_in(mfcc, frames, word_start, mdl_start, cen, cen_frames)
        E, M = int(word_start[-1]), int(mdl_start[-1])
        assert M == cen.shape[0]
        out, assign = np.zeros_like(cen), np.zeros(E, np.uint32)
        stats, it = np.zeros((n_iter, M), TRAIN_STAT_DTYPE), np.zeros(n_iter, CLUSTER_ITER_DTYPE)
        self._check(self.L.sr_cluster_models_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), _vp(word_start), _vp(mdl_start),
                                                C.c_uint32(len(word_start) - 1), _vp(cen), _vp(cen_frames), C.c_uint32(cen.shape[1]),
                                                C.c_uint32(n_iter), _vp(out), _vp(assign), _vp(stats), _vp(it)))
        return out, assign, stats, it

    def cluster_models_dev(self, mfcc, frames, word_start, mdl_start, cen_in, cen_frames, cen_out, n_iter=4, assign=None, stats=None,
                           iters=None, frames_stride=1, stream=None):
        """sr_cluster_models_dp_dev on device tensors (word_start / mdl_start: HOST sequences): cen_in / cen_out int16
        [M, cen_rows, 12], assign (optional) int32 [E], stats (optional) n_iter * M * 16 bytes, iters (optional) n_iter * 24
        bytes.  One asynchronous operation on `stream`; returns cen_out."""
        import torch
        word_start = np.ascontiguousarray(word_start, dtype=np.uint32)
        mdl_start = np.ascontiguousarray(mdl_start, dtype=np.uint32)
        E, M = int(word_start[-1]), int(mdl_start[-1])
        assert mfcc.is_cuda and mfcc.is_contiguous() and cen_in.is_contiguous() and cen_out.is_contiguous()
        assert len(word_start) == len(mdl_start) and E <= mfcc.shape[0] and M == cen_in.shape[0] and cen_out.shape == cen_in.shape
        assert assign is None or (assign.is_contiguous() and assign.numel() == E)
        assert stats is None or (stats.is_contiguous() and stats.numel() * stats.element_size() == n_iter * M * 16)
        assert iters is None or (iters.is_contiguous() and iters.numel() * iters.element_size() == n_iter * 24)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_cluster_models_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), _vp(word_start),
                                                    _vp(mdl_start), C.c_uint32(len(word_start) - 1), _vp(cen_in), _vp(cen_frames),
                                                    C.c_uint32(cen_in.shape[1]), C.c_uint32(n_iter), _vp(cen_out), _vp(assign), _vp(stats),
                                                    _vp(iters), C.c_void_p(stream)))
        return cen_out

    def cluster_words(self, mfcc, frames, labels, n_clusters=4, n_iter=4, init=None):
        """Several templates per word from labelled examples.  The rows are grouped by label (ascending label, rows of a word in
        their order); word w gets min(n_clusters, its example count) models.  Cluster c of C starts from the word's example at
        position ((2c + 1) * n) // (2C) of its n examples in stable ascending order of frame count -- duration is the variation
        the 1/2..2x gate cannot bridge, so the seeds span it -- or from init = (centroids int16 [M, rows, 12], frames [M]) in
        that model order; cluster_models refines them.  Returns (centroids int16 [M, rows, 12], frames uint32 [M], word_ids
        uint32 [M], valid uint8 [M] = received an example in the last iteration, assign uint32 [E] in INPUT order):
        set_templates_dense(centroids, frames, valid) and set_word_map(word_ids) make them the store."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.minimum(np.ascontiguousarray(frames, dtype=np.uint32), self.max_frames)
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        assert len(labels) == len(frames) == mfcc.shape[0] and 1 <= n_clusters <= CLUSTER_MAX
        words, counts = np.unique(labels, return_counts=True)
        order = np.argsort(labels, kind="stable")
        word_start = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
        n_mdl = np.minimum(counts, n_clusters)
        mdl_start = np.concatenate(([0], np.cumsum(n_mdl))).astype(np.uint32)
        word_ids = np.repeat(words, n_mdl).astype(np.uint32)
        if init is None:
            seeds = []
            for w in range(len(words)):
                rows = order[word_start[w]:word_start[w + 1]]
                by_len = rows[np.argsort(frames[rows], kind="stable")]
                n, Cw = len(rows), int(n_mdl[w])
                seeds += [int(by_len[((2 * c + 1) * n) // (2 * Cw)]) for c in range(Cw)]
            cen_frames = frames[seeds]
            cen = np.zeros((len(seeds), max(int(cen_frames.max()), 1) + 1, N_COEF), np.int16)  # (one row of slack, as a store has)
            for m, e in enumerate(seeds):
                cen[m, :cen_frames[m]] = mfcc[e, :cen_frames[m]]
        else:
            cen, cen_frames = np.ascontiguousarray(init[0], dtype=np.int16), np.ascontiguousarray(init[1], dtype=np.uint32)
            assert cen.shape[0] == len(word_ids) == len(cen_frames)
        out, assign, stats, _ = self.cluster_models(mfcc[order], frames[order], word_start, mdl_start, cen, cen_frames, n_iter)
        by_input = np.empty_like(assign)
        by_input[order] = assign
        return out, cen_frames.copy(), word_ids, (stats[-1]["n_ok"] > 0).astype(np.uint8), by_input

    # ---- forced alignment against a transcript: word models trained on connected speech ------------------------
    @staticmethod
    def _transcripts(transcripts, n_rows):
        """a list of label lists -> (labels uint32 [n_rows, words_per_row] padded with NO_WORD, counts uint32 [n_rows])"""
        assert len(transcripts) == n_rows
        counts = np.array([len(t) for t in transcripts], np.uint32)
        W = max(1, int(counts.max(initial=0)))
        labels = np.full((n_rows, W), NO_WORD, np.uint32)
        for r, t in enumerate(transcripts):
            labels[r, :len(t)] = np.asarray(t, np.uint32)
        return labels, counts

    def align_transcripts(self, mfcc, frames, transcripts, skip_cost=None, word_cost=0):
        """OPT-IN (sr_align_transcripts_dp): every feature row aligned to ITS OWN transcript, transcripts = one list of word
        labels (of the word map) per row, up to 16 words; the connected-word decoder's parse with the word sequence given.
        mfcc int16 [n_rows, max_frames, 12], frames uint32 [n_rows].  Returns (rec CHAIN_REC_DTYPE [n_rows], words
        CHAIN_WORD_DTYPE [n_rows, words_per_row]) with words_per_row = the longest transcript (1 at least); `reserved` of a
        word row is the word's 1-based position; a row without a parse (or with an empty transcript) has status CH_NONE."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        assert len(frames) == n
        labels, counts = self._transcripts(transcripts, n)
        W = labels.shape[1]
        rec, words = np.zeros(n, dtype=CHAIN_REC_DTYPE), np.zeros((n, W), dtype=CHAIN_WORD_DTYPE)
        self._check(self.L.sr_align_transcripts_dp(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), _vp(labels), _vp(counts),
                                                   C.c_uint32(W), C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(rec),
                                                   _vp(words)))
        return rec, words

    def align_transcripts_dev(self, mfcc, frames, transcripts, rec, words, skip_cost=None, word_cost=0, frames_stride=1, stream=None):
        """sr_align_transcripts_dp_dev on device tensors (transcripts: a HOST list of label lists): mfcc int16 [n_rows,
        max_frames, 12]; frames as for decode_words_dev; rec int32 [n_rows, 4]; words int32 [n_rows, words_per_row, 8] with
        words_per_row = the size of `words` (the longest transcript at least).  One asynchronous operation on `stream`;
        returns (rec, words)."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and rec.is_contiguous() and words.is_contiguous()
        n = mfcc.shape[0]
        labels, counts = self._transcripts(transcripts, n)
        W = words.numel() // (n * 8) if n else labels.shape[1]
        assert rec.numel() == n * 4 and words.numel() == n * W * 8 and W >= labels.shape[1]
        if W > labels.shape[1]:
            labels = np.concatenate([labels, np.full((n, W - labels.shape[1]), NO_WORD, np.uint32)], axis=1)
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_align_transcripts_dp_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n),
                                                       _vp(np.ascontiguousarray(labels)), _vp(counts), C.c_uint32(W),
                                                       C.c_uint32(self._skip(skip_cost)), C.c_uint32(word_cost), _vp(rec), _vp(words),
                                                       C.c_void_p(stream)))
        return rec, words

    def gather_word_spans(self, mfcc, frames, words, dst_of_span, n_ex, ex_rows):
        """OPT-IN (sr_gather_word_spans): word spans cut out of feature rows into the trainers' example layout.  words
        CHAIN_WORD_DTYPE [n_rows, words_per_row] (any decoder's; start and end are read); dst_of_span uint32 [n_rows *
        words_per_row] = the example each span goes to (distinct indices below n_ex) or NO_WORD for "not wanted".  Returns (ex
        int16 [n_ex, ex_rows, 12], ex_frames uint32 [n_ex]); an invalid or too long span and an unnamed example are empty rows."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        words = np.ascontiguousarray(words, dtype=CHAIN_WORD_DTYPE).reshape(n, -1) if n else np.zeros((0, 1), CHAIN_WORD_DTYPE)
        dst = np.ascontiguousarray(dst_of_span, dtype=np.uint32)
        assert len(frames) == n and dst.size == words.size
        ex, ex_frames = np.zeros((n_ex, max(ex_rows, 0), N_COEF), np.int16), np.zeros(n_ex, np.uint32)
        self._check(self.L.sr_gather_word_spans(self.h, _vp(mfcc), _vp(frames), C.c_uint32(1), C.c_uint32(n), _vp(words),
                                                C.c_uint32(words.shape[1]), _vp(dst), C.c_uint32(n_ex), C.c_uint32(ex_rows), _vp(ex),
                                                _vp(ex_frames)))
        return ex, ex_frames

    def gather_word_spans_dev(self, mfcc, frames, words, dst_of_span, ex, ex_frames, frames_stride=1, stream=None):
        """sr_gather_word_spans_dev on device tensors (dst_of_span: a HOST sequence): words int32 [n_rows, words_per_row, 8];
        ex int16 [n_ex, ex_rows, 12]; ex_frames int32 [n_ex].  One asynchronous operation on `stream`; returns (ex, ex_frames)."""
        import torch
        assert mfcc.is_cuda and mfcc.is_contiguous() and words.is_contiguous() and ex.is_contiguous() and ex_frames.is_contiguous()
        n, n_ex = mfcc.shape[0], ex.shape[0]
        dst = np.ascontiguousarray(dst_of_span, dtype=np.uint32)
        assert n and words.numel() % (n * 8) == 0 and dst.size * 8 == words.numel() and ex_frames.numel() == n_ex and ex.shape[2] == N_COEF
        if stream is None:
            stream = torch.cuda.current_stream(mfcc.device).cuda_stream
        self._check(self.L.sr_gather_word_spans_dev(self.h, _vp(mfcc), _vp(frames), C.c_uint32(frames_stride), C.c_uint32(n), _vp(words),
                                                    C.c_uint32(words.numel() // (n * 8)), _vp(dst), C.c_uint32(n_ex), C.c_uint32(ex.shape[1]),
                                                    _vp(ex), _vp(ex_frames), C.c_void_p(stream)))
        return ex, ex_frames

    def train_connected(self, mfcc, frames, transcripts, n_iter=4, skip_cost=None, word_cost=0, ex_rows=None):
        """Embedded re-estimation of the word models from CONNECTED recordings with known transcripts.  The current store
        (set_templates_dense) and word map are the starting models.  Per iteration: align_transcripts against the store; gather
        every transcript word as an example (grouped by word in word_groups order, inside a word by (row, position)); one
        cluster_models iteration with all slots of a word as that word's models (an invalid slot is a centroid of 0 frames,
        copied through; a word with one slot is plain DBA); set_templates_dense with the new centroids -- valid flags, frame
        counts and the word map stay.  The store is set from host memory, so the centroids are read back once per iteration.
        ex_rows: rows of an example (None: min(max_frames, ALIGN_MAX_FRAMES)); a longer span is dropped.  A word with more
        than CLUSTER_MAX slots is refused.  Returns (centroids int16 [K, rows, 12], frames uint32 [K], iters = a list of (OK
        rows, the sum of their rec.cost) per iteration, words = the last alignment's word rows)."""
        if self._tpl is None or self._tpl[0] != "set_templates_dense":
            raise SrError("train_connected needs a store set with set_templates_dense")
        tm, tf, valid = self._tpl[1]
        K = tm.shape[0]
        wmap = getattr(self, "_wmap", (None, 1))
        lab = np.arange(K, dtype=np.uint32) // wmap[1] if wmap[0] is None else wmap[0]
        assert len(lab) == K, "the word map does not fit the template store"
        grp = self.word_groups(words=lab)
        order, gstart, ids = grp["order"], grp["group_start"], grp["word_id"]
        if int(np.diff(gstart.astype(np.int64)).max()) > CLUSTER_MAX:
            raise SrError(f"train_connected: a word with more than {CLUSTER_MAX} slots")
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        n = mfcc.shape[0]
        labels, counts = self._transcripts(transcripts, n)
        W = labels.shape[1]
        # the example layout: the host knows it from the transcripts alone
        dst = np.full(n * W, NO_WORD, np.uint32)
        word_start, e = [0], 0
        for w in ids:
            at = np.nonzero((labels == w) & (np.arange(W)[None, :] < counts[:, None]))
            for r, i in zip(*at):  # (row-major: ascending row, then position)
                dst[r * W + i] = e
                e += 1
            word_start.append(e)
        word_start = np.array(word_start, np.uint32)
        ex_rows = min(self.max_frames, ALIGN_MAX_FRAMES) if ex_rows is None else int(ex_rows)
        trainer = self  # the clustering calls take example rows of THEIR engine's max_frames; they touch no store
        if ex_rows != self.max_frames:
            trainer = Engine(max_frames=ex_rows, device=self.cfg.device, testing=self._testing, **self._kw)
        cen_frames = np.where(valid[order] != 0, tf[order], 0).astype(np.uint32) if valid is not None else tf[order].astype(np.uint32)
        iters, words = [], None
        try:
            for _ in range(n_iter):
                rec, words = self.align_transcripts(mfcc, frames, transcripts, skip_cost, word_cost)
                ok = rec["status"] == 0
                iters.append((int(ok.sum()), int(rec["cost"][ok].astype(np.int64).sum())))
                ex, ex_frames = self.gather_word_spans(mfcc, frames, words, dst, e, ex_rows)
                cen, _, _, _ = trainer.cluster_models(ex, ex_frames, word_start, gstart, tm[order], cen_frames, 1)
                tm = tm.copy()
                tm[order] = cen
                self.set_templates_dense(tm, tf, valid)
        finally:
            if trainer is not self:
                trainer.close()
        return tm, tf.copy(), iters, words

    def get_mdl(self, in1, n1, in2, n2, mdl_rows):
        """get_mdl (DTW.C:217-296) on P pairs: in1 int16 [P, rows1, 12], in2 int16 [P, rows2, 12].
        Returns (mdl int16 [P, mdl_rows, 12], mdl_frames uint32 [P], dis uint32 [P])."""
        in1 = np.ascontiguousarray(in1, dtype=np.int16)
        in2 = np.ascontiguousarray(in2, dtype=np.int16)
        n1 = np.ascontiguousarray(n1, dtype=np.uint32)
        n2 = np.ascontiguousarray(n2, dtype=np.uint32)
        P = in1.shape[0]
        assert in1.shape[2] == N_COEF and in2.shape[2] == N_COEF and in2.shape[0] == P
        mdl = np.zeros((P, mdl_rows, N_COEF), dtype=np.int16)
        frames = np.zeros(P, dtype=np.uint32)
        dis = np.zeros(P, dtype=np.uint32)
        self._check(self.L.sr_get_mdl_batch(self.h, _vp(in1), _vp(n1), C.c_uint32(in1.shape[1]), _vp(in2), _vp(n2),
                                            C.c_uint32(in2.shape[1]), C.c_uint32(P), _vp(mdl), C.c_uint32(mdl_rows),
                                            _vp(frames), _vp(dis)))
        return mdl, frames, dis

    def delta_mfcc(self, mfcc, frames):
        """EXTENSION (no reference counterpart): two-frame regression delta cepstra of B records [B, max_frames, 12]."""
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        assert mfcc.shape[1:] == (self.max_frames, self.n_coef)
        out = np.zeros_like(mfcc)
        self._check(self.L.sr_delta_mfcc_batch(self.h, _vp(mfcc), _vp(frames), C.c_uint32(len(frames)), _vp(out)))
        return out

    def fft_q15(self, words):
        """cr4_fft_1024_stm32 on uint32 [n, 1024] packed complex arrays."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        out = np.zeros_like(words)
        self._check(self.L.sr_fft_q15_batch(self.h, _vp(words), _vp(out), C.c_uint32(words.shape[0])))
        return out

    # ---- device-resident API (torch tensors as HBM handles) ---------------------------------------------
    def alloc_outputs(self, B, device, scores=True, mfcc=True, vad=True):
        import torch
        K = self.n_templates
        o = dict(results=torch.empty(B, 4, dtype=torch.int32, device=device))
        o["scores"] = torch.empty(B, K, dtype=torch.int32, device=device) if scores else None
        o["mfcc"] = torch.empty(B, self.max_frames, self.n_coef, dtype=torch.int16, device=device) if mfcc else None
        o["vad"] = torch.empty(B, 12, dtype=torch.int32, device=device) if vad else None
        return o

    def recognize_dev(self, pcm, out, buf_len=None, stream=None):
        """pcm: torch int16 [B, S] in HBM holding the u16 ADC codes; out: alloc_outputs().  Asynchronous."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        B, S = pcm.shape
        if stream is None:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
        self._check(self.L.sr_recognize_batch_dev(
            self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S if buf_len is None else buf_len), C.c_uint32(B),
            _vp(out["results"]), _vp(out["scores"]), _vp(out["mfcc"]), _vp(out["vad"]), C.c_void_p(stream)))
        return out

    def recognize_nbest_dev(self, pcm, out, n_best, buf_len=None, stream=None, rescore=False):
        """recognize_dev() plus the n_best best words of every capture (sr_recognize_nbest_batch_dev): out gains
        out["nbest"] int32 [B, n_best, 4] (sr_nbest_entry records; nbest_from_torch()) and out["n_matched"] int32 [B],
        allocated here unless the caller put them there.  rescore=True (sr_recognize_rescored_batch_dev): out also gains
        out["rescored"] int32 [B, n_best, 4] and out["n_rescored"] int32 [B], the second pass of every list; a caller who
        puts out["nbest"] = False there does not get the first-pass list back.  Asynchronous."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        B, S = pcm.shape
        if stream is None:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
        if out.get("nbest") is None:
            out["nbest"] = torch.empty(B, max(n_best, 0), 4, dtype=torch.int32, device=pcm.device)
        if "n_matched" not in out:
            out["n_matched"] = torch.empty(B, dtype=torch.int32, device=pcm.device)
        if rescore:
            if out.get("rescored") is None:
                out["rescored"] = torch.empty(B, max(n_best, 0), 4, dtype=torch.int32, device=pcm.device)
            if "n_rescored" not in out:
                out["n_rescored"] = torch.empty(B, dtype=torch.int32, device=pcm.device)
            first = None if out["nbest"] is False else out["nbest"]
            self._check(self.L.sr_recognize_rescored_batch_dev(
                self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S if buf_len is None else buf_len), C.c_uint32(B), C.c_uint32(n_best),
                _vp(first), _vp(out["n_matched"]), _vp(out["rescored"]), _vp(out["n_rescored"]), _vp(out["results"]),
                _vp(out["scores"]), _vp(out["mfcc"]), _vp(out["vad"]), C.c_void_p(stream)))
            return out
        self._check(self.L.sr_recognize_nbest_batch_dev(
            self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S if buf_len is None else buf_len), C.c_uint32(B), C.c_uint32(n_best),
            _vp(out["nbest"]), _vp(out["n_matched"]), _vp(out["results"]), _vp(out["scores"]), _vp(out["mfcc"]),
            _vp(out["vad"]), C.c_void_p(stream)))
        return out

    def features_dev(self, pcm, buf_len=None, stream=None):
        """VAD + MFCC only (template creation = the same front end, main.c:121-138).
        Returns (vad [B,12] int32, mfcc [B,max_frames,12] int16) device tensors."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        B, S = pcm.shape
        if stream is None:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
        vad = torch.empty(B, 12, dtype=torch.int32, device=pcm.device)
        mfcc = torch.empty(B, self.max_frames, self.n_coef, dtype=torch.int16, device=pcm.device)
        self._check(self.L.sr_vad_batch_dev(self.h, _vp(pcm), C.c_uint64(S),
                                            C.c_uint32(S if buf_len is None else buf_len), C.c_uint32(B), _vp(vad),
                                            C.c_void_p(stream)))
        self._check(self.L.sr_mfcc_batch_dev(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(B), _vp(vad), _vp(mfcc),
                                             C.c_void_p(stream)))
        return vad, mfcc

    def frame_features_dev(self, pcm, vad, kind, mfcc=None, stream=None):
        """sr_frame_features_batch_dev on device tensors: pcm int16 [B, S] (u16 codes), vad [B, 12] int32 records (from
        features_dev / recognize_dev); mfcc (optional) int16 [B, max_frames, n_coef] receives the MFCC rows of the same
        launch.  Returns the feature tensor int32 [B, max_frames, width] (the u32 words; .view(torch.uint32) or numpy
        .view(np.uint32) to read them unsigned).  Asynchronous on `stream` (a torch.cuda.Stream, or the current one)."""
        import torch
        assert pcm.is_cuda and pcm.dtype in (torch.int16, torch.uint16) and pcm.is_contiguous()
        B, S = pcm.shape
        width = self.frame_feature_width(kind)
        if stream is None:
            stream = torch.cuda.current_stream(pcm.device)
        feat = torch.empty(B, self.max_frames, max(width, 1), dtype=torch.int32, device=pcm.device)
        self._check(self.L.sr_frame_features_batch_dev(self.h, C.c_int(kind), _vp(pcm), C.c_uint64(S), C.c_uint32(B),
                                                       _vp(vad), _vp(feat), _vp(mfcc),
                                                       C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            feat.record_stream(stream)  # allocated on the current stream, written on `stream`
        return feat

    def recognize_stream_dev(self, pcm, max_segs, lengths=None, atap=None, scores=True, mfcc=True, stream=None, n_best=None):
        """sr_recognize_stream_dev on device tensors: pcm int16 [B, S] (u16 codes), lengths int32 [B] (or None), atap
        int32 [B, 3] sr_atap records (or None).  Asynchronous on `stream` (a torch.cuda.Stream, or the current one).
        Returns dict of device tensors: segs int32 [max_segs, 4], seg_offsets int32 [B+1] (the last = the true total),
        results int32 [max_segs, 4], scores [max_segs, K], mfcc [max_segs, max_frames, n_coef].  n_best:
        sr_recognize_stream_nbest_dev, plus nbest int32 [max_segs, n_best, 4] and n_matched int32 [max_segs]."""
        import torch
        assert pcm.is_cuda and pcm.dtype in (torch.int16, torch.uint16) and pcm.is_contiguous()
        B, S = pcm.shape
        dev, K = pcm.device, self.n_templates
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        o = dict(segs=torch.empty(max(max_segs, 1), 4, dtype=torch.int32, device=dev)[:max_segs],
                 seg_offsets=torch.empty(B + 1, dtype=torch.int32, device=dev),
                 results=torch.empty(max(max_segs, 1), 4, dtype=torch.int32, device=dev)[:max_segs])
        o["scores"] = torch.empty(max_segs, K, dtype=torch.int32, device=dev) if scores else None
        o["mfcc"] = torch.empty(max_segs, self.max_frames, self.n_coef, dtype=torch.int16, device=dev) if mfcc else None
        head = (self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), _vp(lengths), C.c_uint32(B), _vp(atap), C.c_uint32(max_segs),
                _vp(o["segs"]), _vp(o["seg_offsets"]))
        tail = (_vp(o["results"]), _vp(o["scores"]), _vp(o["mfcc"]), C.c_void_p(getattr(stream, "cuda_stream", stream)))
        if n_best is None:
            self._check(self.L.sr_recognize_stream_dev(*head, *tail))
        else:
            o["nbest"] = torch.empty(max(max_segs, 1), max(n_best, 0), 4, dtype=torch.int32, device=dev)[:max_segs]
            o["n_matched"] = torch.empty(max(max_segs, 1), dtype=torch.int32, device=dev)[:max_segs]
            self._check(self.L.sr_recognize_stream_nbest_dev(*head, C.c_uint32(n_best), _vp(o["nbest"]), _vp(o["n_matched"]),
                                                             *tail))
        if isinstance(stream, torch.cuda.Stream):
            for t in o.values():
                if t is not None:
                    t.record_stream(stream)  # allocated on the current stream, written on `stream`
        return o

    def live(self, n_channels, chunk_max, atap=None):
        """sr_live_open: a LiveSession of n_channels channels taking pushes of at most chunk_max samples per channel; atap
        None (noise_atap over each channel's head) or an ATAP_DTYPE array [n_channels].  Close it before the engine."""
        return LiveSession(self, n_channels, chunk_max, atap)

    def spot_live(self, n_channels, chunk_max, win_frames, mid=None):
        """sr_spot_live_open: a SpotSession of n_channels channels with windows of win_frames end frames.  mid None: a feature
        session taking pushes of at most chunk_max frames per channel; mid uint32 [n_channels]: a PCM session, chunk_max in
        samples.  Close it before the engine."""
        return SpotSession(self, n_channels, chunk_max, win_frames, mid)

    def set_pipeline(self, streams=3, min_chunk=4096, max_chunks=12):
        """chunking of recognize_dev over the engine's internal streams (streams=1: one chunk, caller's stream)"""
        self._check(self.L.sr_set_pipeline(self.h, C.c_uint32(streams), C.c_uint32(min_chunk), C.c_uint32(max_chunks)))

    def set_profiling(self, on=True):
        self._check(self.L.sr_set_profiling(self.h, C.c_int(1 if on else 0)))

    def stage_ms(self):
        ms = (C.c_float * 5)()
        self._check(self.L.sr_get_stage_ms(self.h, ms))
        n = C.c_uint32(0)
        self._check(self.L.sr_get_stage_launches(self.h, C.byref(n)))
        return dict(vad=ms[0], mfcc=ms[1], dtw=ms[2], argmin=ms[3], total=ms[4], launches_per_call=n.value)


def spot_geometry(tpl_rows, max_frames, win_frames=0, testing=False):
    """Host-only sr_spot_geometry: dict(n_win, lds_bytes of one workgroup for a store whose longest template has tpl_rows
    rows, max_tpl_rows that fit, chunk_cols = end frames per kernel chunk)."""
    L = load_library(testing)
    out = (C.c_uint32 * 4)()
    rc = L.sr_spot_geometry(C.c_uint32(tpl_rows), C.c_uint32(max_frames), C.c_uint32(win_frames), out)
    if rc != 0:
        raise SrError(f"sr_spot_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(n_win=out[0], lds_bytes=out[1], max_tpl_rows=out[2], chunk_cols=out[3])


def decode_geometry(tpl_rows, max_frames, max_words=8, testing=False):
    """Host-only sr_decode_geometry: dict(scratch_bytes per row for the levels' keys and prefix costs, rows per launch group,
    max_tpl_rows that fit, chunk_cols = end frames per kernel chunk)."""
    L = load_library(testing)
    out = (C.c_uint32 * 4)()
    rc = L.sr_decode_geometry(C.c_uint32(tpl_rows), C.c_uint32(max_frames), C.c_uint32(max_words), out)
    if rc != 0:
        raise SrError(f"sr_decode_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(scratch_bytes=out[0], rows=out[1], max_tpl_rows=out[2], chunk_cols=out[3])


def decode_onepass_geometry(tpl_rows, n_templates, max_frames, min_tpl_frames, testing=False):
    """Host-only sr_decode_onepass_geometry for a store of n_templates slots whose longest template has tpl_rows rows and whose
    shortest valid one min_tpl_frames frames: dict(state_bytes per row for keys, prefix costs and saved columns, rows per
    launch group, block = frames per block (min_tpl_frames // 2 + 1), launches per group)."""
    L = load_library(testing)
    out = (C.c_uint32 * 4)()
    rc = L.sr_decode_onepass_geometry(C.c_uint32(tpl_rows), C.c_uint32(n_templates), C.c_uint32(max_frames), C.c_uint32(min_tpl_frames), out)
    if rc != 0:
        raise SrError(f"sr_decode_onepass_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(state_bytes=out[0], rows=out[1], block=out[2], launches=out[3])


def align_geometry(max_frames, ref_rows, testing=False):
    """Host-only sr_align_geometry: dict(scratch_bytes per pair for the predecessor marks (0: they live in LDS), pairs per
    launch, max_frames = SR_ALIGN_MAX_FRAMES)."""
    L = load_library(testing)
    out = (C.c_uint32 * 3)()
    rc = L.sr_align_geometry(C.c_uint32(max_frames), C.c_uint32(ref_rows), out)
    if rc != 0:
        raise SrError(f"sr_align_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(scratch_bytes=out[0], pairs=out[1], max_frames=out[2])


def live_geometry(chunk_max, max_frames=119, **kw):
    """Host-only sr_live_geometry for a configuration (keywords as Engine's): (ring samples per channel, most records one
    channel can emit in one push of chunk_max samples, device bytes per channel)"""
    L = load_library()
    cfg = Config()
    L.sr_default_config(C.byref(cfg))
    cfg.max_frames = max_frames
    for k, v in kw.items():
        setattr(cfg, k, v)
    out = (C.c_uint32 * 3)()
    rc = L.sr_live_geometry(C.byref(cfg), C.c_uint32(chunk_max), out)
    if rc != 0:
        raise SrError(f"sr_live_geometry error {rc}: {L.sr_last_error().decode()}")
    return tuple(out)


class LiveSession:
    """One sr_live handle (Engine.live): chunked audio on n_channels channels, VAD state carried between pushes.  The records
    of a channel, over any chunking, are those of Engine.recognize_stream on everything pushed to it (include/sr_engine.h)."""

    def __init__(self, eng, n_channels, chunk_max, atap=None):
        self.eng, self.L, self.n_channels, self.chunk_max = eng, eng.L, n_channels, chunk_max
        self.L.sr_live_event_bound.restype = C.c_uint32
        self.L.sr_live_close.restype = None
        self.L.sr_live_close.argtypes = [C.c_void_p]
        at = None if atap is None else np.ascontiguousarray(atap, dtype=ATAP_DTYPE)
        assert at is None or len(at) == n_channels
        l = C.c_void_p()
        eng._check(self.L.sr_live_open(eng.h, C.c_uint32(n_channels), C.c_uint32(chunk_max), _vp(at), C.byref(l)))
        self.l = l

    def close(self):
        if getattr(self, "l", None):
            self.L.sr_live_close(self.l)
            self.l = None

    def __del__(self):
        try:
            if getattr(self.eng, "h", None):  # a session never outlives its engine's handle
                self.close()
        except Exception:
            pass

    def _counts(self, counts, width):
        """(host uint32 array or None, n_all)"""
        if counts is None:
            return None, width
        ct = np.ascontiguousarray(counts, dtype=np.uint32)
        assert ct.shape == (self.n_channels,)
        return ct, 0

    def event_bound(self, counts):
        """sr_live_event_bound: most records a push with these counts (an int: that many on every channel) can emit"""
        if np.isscalar(counts):
            return int(self.L.sr_live_event_bound(self.l, None, C.c_uint32(int(counts))))
        ct, _ = self._counts(counts, 0)
        return int(self.L.sr_live_event_bound(self.l, _vp(ct), C.c_uint32(0)))

    def push(self, chunks, counts=None, n_best=None, want_scores=True, want_mfcc=True, recognize=True, max_segs=None):
        """sr_live_push: chunks uint16 [n_channels, W], counts [n_channels] (None: W each).  Returns dict(segs
        LIVE_SEG_DTYPE [n], total = n, results, scores, mfcc[, nbest, n_matched]) of numpy arrays."""
        pcm = np.ascontiguousarray(chunks, dtype=np.uint16)
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_channels
        W = pcm.shape[1]
        ct, n_all = self._counts(counts, W)
        if max_segs is None:
            max_segs = self.event_bound(W if ct is None else ct)
        eng = self.eng
        K = eng.n_templates if recognize else 0
        segs = np.zeros(max_segs, dtype=LIVE_SEG_DTYPE)
        res = np.zeros(max_segs, dtype=RESULT_DTYPE) if recognize else None
        sc = np.zeros((max_segs, K), dtype=np.uint32) if recognize and want_scores else None
        mf = np.zeros((max_segs, eng.max_frames, eng.n_coef), dtype=np.int16) if recognize and want_mfcc else None
        nb = nm = None
        if recognize and n_best is not None:
            nb = np.zeros((max_segs, max(n_best, 0)), dtype=NBEST_DTYPE)
            nm = np.zeros(max_segs, dtype=np.uint32)
        total = C.c_uint32(0)
        eng._check(self.L.sr_live_push(self.l, _vp(pcm), C.c_uint64(max(W, 1)), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_segs),
                                       _vp(segs), C.c_uint32(n_best if nb is not None else 0), _vp(nb), _vp(nm), _vp(res), _vp(sc),
                                       _vp(mf), C.byref(total)))
        cut = (lambda x: None if x is None else x[:total.value])
        out = dict(segs=cut(segs), total=total.value, results=cut(res), scores=cut(sc), mfcc=cut(mf))
        if nb is not None:
            out.update(nbest=cut(nb), n_matched=cut(nm))
        return out

    def push_dev(self, chunks, counts=None, n_best=None, scores=True, mfcc=True, recognize=True, max_segs=None, stream=None):
        """sr_live_push_dev on a device tensor: chunks int16 [n_channels, W] (u16 codes, W a multiple of 8), counts a HOST
        array [n_channels] (None: W each).  Asynchronous on `stream` (a torch.cuda.Stream, or the current one).  Returns a
        dict of device tensors max_segs long: segs int32 [max_segs, 6] (sr_live_seg records), count int32 [1], results,
        scores, mfcc[, nbest, n_matched]; rows at and past count are padding."""
        import torch
        assert chunks.is_cuda and chunks.dtype in (torch.int16, torch.uint16) and chunks.is_contiguous()
        assert chunks.shape[0] == self.n_channels
        W = chunks.shape[1]
        ct, n_all = self._counts(counts, W)
        if max_segs is None:
            max_segs = self.event_bound(W if ct is None else ct)
        eng, dev = self.eng, chunks.device
        K = eng.n_templates if recognize else 0
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        rows = max(max_segs, 1)
        o = dict(segs=torch.empty(rows, 6, dtype=torch.int32, device=dev)[:max_segs],
                 count=torch.empty(1, dtype=torch.int32, device=dev))
        o["results"] = torch.empty(rows, 4, dtype=torch.int32, device=dev)[:max_segs] if recognize else None
        o["scores"] = torch.empty(max_segs, K, dtype=torch.int32, device=dev) if recognize and scores else None
        o["mfcc"] = torch.empty(max_segs, eng.max_frames, eng.n_coef, dtype=torch.int16, device=dev) if recognize and mfcc else None
        nb = nm = None
        if recognize and n_best is not None:
            nb = o["nbest"] = torch.empty(rows, max(n_best, 0), 4, dtype=torch.int32, device=dev)[:max_segs]
            nm = o["n_matched"] = torch.empty(rows, dtype=torch.int32, device=dev)[:max_segs]
        eng._check(self.L.sr_live_push_dev(self.l, _vp(chunks), C.c_uint64(W), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_segs),
                                           _vp(o["segs"]), _vp(o["count"]), C.c_uint32(n_best if nb is not None else 0), _vp(nb),
                                           _vp(nm), _vp(o["results"]), _vp(o["scores"]), _vp(o["mfcc"]),
                                           C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            chunks.record_stream(stream)
            for t in o.values():
                if t is not None:
                    t.record_stream(stream)  # allocated on the current stream, written on `stream`
        return o

    def end(self, channels):
        """sr_live_end: the listed channels' recordings end here.  Returns the LIVE_SEG_DTYPE records {start, -1} of those
        that were inside a segment; afterwards the channels are as freshly opened."""
        ch = np.ascontiguousarray(np.atleast_1d(channels), dtype=np.uint32)
        segs = np.zeros(max(len(ch), 1), dtype=LIVE_SEG_DTYPE)
        n = C.c_uint32(0)
        self.eng._check(self.L.sr_live_end(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(segs), C.byref(n)))
        return segs[:n.value]


def spot_live_geometry(tpl_rows, K, chunk_max, win_frames):
    """Host-only sr_spot_live_geometry: dict(max_windows one channel can complete in one push of chunk_max frames, state_bytes
    on the device per channel, max_tpl_rows that fit)"""
    L = load_library()
    out = (C.c_uint32 * 3)()
    rc = L.sr_spot_live_geometry(C.c_uint32(tpl_rows), C.c_uint32(K), C.c_uint32(chunk_max), C.c_uint32(win_frames), out)
    if rc != 0:
        raise SrError(f"sr_spot_live_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(max_windows=out[0], state_bytes=out[1], max_tpl_rows=out[2])


def spot_live_windows(win_frames, frames_before, n_new):
    """Host-only sr_spot_live_windows: the window rows a push emits when channel c stands at frames_before[c] frames and gets
    n_new[c] more (what SpotSession.rows computes from the session's own counts)"""
    L = load_library()
    L.sr_spot_live_windows.restype = C.c_uint32
    fb, nn = np.ascontiguousarray(frames_before, dtype=np.uint32), np.ascontiguousarray(n_new, dtype=np.uint32)
    assert fb.shape == nn.shape and fb.ndim == 1
    return int(L.sr_spot_live_windows(C.c_uint32(win_frames), _vp(fb), _vp(nn), C.c_uint32(len(fb))))


class SpotSession:
    """One sr_spot_live handle (Engine.spot_live): word spotting over chunked features or samples on n_channels channels, the
    spotter's state carried between pushes.  The records of a channel's windows, over any chunking, are those of Engine.spot
    on everything pushed to it as one row (include/sr_engine.h, "live word spotting")."""

    def __init__(self, eng, n_channels, chunk_max, win_frames, mid=None):
        self.eng, self.L, self.n_channels, self.chunk_max, self.win_frames = eng, eng.L, n_channels, chunk_max, win_frames
        self.L.sr_spot_live_rows.restype = C.c_uint32
        self.L.sr_spot_live_close.restype = None
        self.L.sr_spot_live_close.argtypes = [C.c_void_p]
        md = None if mid is None else np.ascontiguousarray(mid, dtype=np.uint32)
        assert md is None or md.shape == (n_channels,)
        self.pcm = md is not None
        l = C.c_void_p()
        eng._check(self.L.sr_spot_live_open(eng.h, C.c_uint32(n_channels), C.c_uint32(chunk_max), C.c_uint32(win_frames), _vp(md),
                                            C.byref(l)))
        self.l = l

    def close(self):
        if getattr(self, "l", None):
            self.L.sr_spot_live_close(self.l)
            self.l = None

    def __del__(self):
        try:
            if getattr(self.eng, "h", None):  # a session never outlives its engine's handle
                self.close()
        except Exception:
            pass

    def _counts(self, counts, width):
        """(host uint32 array or None, n_all)"""
        if counts is None:
            return None, width
        ct = np.ascontiguousarray(counts, dtype=np.uint32)
        assert ct.shape == (self.n_channels,)
        return ct, 0

    def rows(self, counts):
        """sr_spot_live_rows: the exact number of window rows a push with these counts (an int: that many on every channel)
        emits"""
        if np.isscalar(counts):
            return int(self.L.sr_spot_live_rows(self.l, None, C.c_uint32(int(counts))))
        ct, _ = self._counts(counts, 0)
        return int(self.L.sr_spot_live_rows(self.l, _vp(ct), C.c_uint32(0)))

    def _push_host(self, fn, data, stride, width, counts, max_rows):
        ct, n_all = self._counts(counts, width)
        if max_rows is None:
            max_rows = self.rows(width if ct is None else ct)
        K = self.eng.n_templates
        hits, sc = np.zeros((max_rows, K), dtype=SPOT_DTYPE), np.zeros((max_rows, K), dtype=np.uint32)
        wins, n = np.zeros(max_rows, dtype=SPOT_WIN_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(hits), _vp(sc),
                           _vp(wins), C.byref(n)))
        return dict(hits=hits[:n.value], scores=sc[:n.value], wins=wins[:n.value], n_rows=n.value)

    def _push_dev(self, fn, data, stride, width, counts, max_rows, scores, stream):
        import torch
        ct, n_all = self._counts(counts, width)
        if max_rows is None:
            max_rows = self.rows(width if ct is None else ct)
        K, dev = self.eng.n_templates, data.device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        rows = max(max_rows, 1)
        hits = torch.empty(rows, K, 4, dtype=torch.int32, device=dev)[:max_rows]
        sc = torch.empty(rows, K, dtype=torch.int32, device=dev)[:max_rows] if scores else None
        wins, n = np.zeros(max_rows, dtype=SPOT_WIN_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(hits), _vp(sc),
                           _vp(wins), C.byref(n), C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            for t in (data, hits, sc):
                if t is not None:
                    t.record_stream(stream)  # allocated on the current stream, used on `stream`
        return dict(hits=hits[:n.value], scores=None if sc is None else sc[:n.value], wins=wins[:n.value], n_rows=n.value)

    def push(self, frames, counts=None, max_rows=None):
        """sr_spot_live_push: frames int16 [n_channels, F, 12], counts [n_channels] (None: F each).  Returns dict(hits SPOT_DTYPE
        [n_rows, K], scores uint32 [n_rows, K], wins SPOT_WIN_DTYPE [n_rows], n_rows) of numpy arrays."""
        mf = np.ascontiguousarray(frames, dtype=np.int16)
        assert mf.ndim == 3 and mf.shape[0] == self.n_channels and mf.shape[2] == N_COEF
        F = mf.shape[1]
        return self._push_host(self.L.sr_spot_live_push, mf, max(F, 1) * N_COEF, F, counts, max_rows)

    def push_dev(self, frames, counts=None, max_rows=None, scores=True, stream=None):
        """sr_spot_live_push_dev on a device tensor: frames int16 [n_channels, F, 12], counts a HOST array [n_channels] (None: F
        each).  Asynchronous on `stream` (a torch.cuda.Stream, or the current one).  Returns dict(hits int32 [n_rows, K, 4],
        scores int32 [n_rows, K] or None -- device tensors, compact over the emitted rows -- wins, n_rows on the host)."""
        import torch
        assert frames.is_cuda and frames.dtype == torch.int16 and frames.is_contiguous()
        assert frames.ndim == 3 and frames.shape[0] == self.n_channels and frames.shape[2] == N_COEF
        F = frames.shape[1]
        return self._push_dev(self.L.sr_spot_live_push_dev, frames, max(F, 1) * N_COEF, F, counts, max_rows, scores, stream)

    def push_pcm(self, chunks, counts=None, max_rows=None):
        """sr_spot_live_push_pcm: chunks uint16 [n_channels, S], counts [n_channels] in samples (None: S each); returns as push"""
        pcm = np.ascontiguousarray(chunks, dtype=np.uint16)
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_channels
        S = pcm.shape[1]
        return self._push_host(self.L.sr_spot_live_push_pcm, pcm, max(S, 1), S, counts, max_rows)

    def push_pcm_dev(self, chunks, counts=None, max_rows=None, scores=True, stream=None):
        """sr_spot_live_push_pcm_dev: chunks int16 [n_channels, S] on the device (u16 codes, S a multiple of 8); returns as
        push_dev"""
        import torch
        assert chunks.is_cuda and chunks.dtype in (torch.int16, torch.uint16) and chunks.is_contiguous()
        assert chunks.ndim == 2 and chunks.shape[0] == self.n_channels
        S = chunks.shape[1]
        return self._push_dev(self.L.sr_spot_live_push_pcm_dev, chunks, S, S, counts, max_rows, scores, stream)

    def end(self, channels):
        """sr_spot_live_end: the listed channels' recordings end here.  Returns dict(hits SPOT_DTYPE [n_rows, K], wins, n_rows):
        the open window of each listed channel that has one; afterwards the channels are as freshly opened."""
        ch = np.ascontiguousarray(np.atleast_1d(channels), dtype=np.uint32)
        K = self.eng.n_templates
        hits = np.zeros((max(len(ch), 1), K), dtype=SPOT_DTYPE)
        wins, n = np.zeros(max(len(ch), 1), dtype=SPOT_WIN_DTYPE), C.c_uint32(0)
        self.eng._check(self.L.sr_spot_live_end(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(hits), _vp(wins), C.byref(n)))
        return dict(hits=hits[:n.value], wins=wins[:n.value], n_rows=n.value)


GRAM_ARC_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("word", "<u4"), ("reserved", "<u4")])  # sr_gram_arc


def grammar_any(labels):
    """The anchor grammar: one state, final, one loop per label -- every sequence of words, byte for byte decode_words().
    Returns (n_states, arcs, final) for Engine.grammar()."""
    return 1, [(0, 0, int(w)) for w in dict.fromkeys(labels)], [1]


def grammar_sequence(positions, optional_tail=False):
    """A linear grammar: word i of a parse is one of the labels positions[i].  The last state is final; optional_tail makes
    every state past the first word final too (the sequence may stop early).  Returns (n_states, arcs, final)."""
    n = len(positions)
    arcs = [(i, i + 1, int(w)) for i, ws in enumerate(positions) for w in dict.fromkeys(ws)]
    return n + 1, arcs, [int(i == n or (optional_tail and i >= 1)) for i in range(n + 1)]


def grammar_word_pairs(labels, allowed_pairs, first=None, last=None):
    """A word-pair grammar: one state per word (1 + its index in labels) plus the start.  A parse may begin with a word of
    `first`, b may follow a when (a, b) is in allowed_pairs, and it may end after a word of `last` (None: any word).
    Returns (n_states, arcs, final)."""
    labels = list(dict.fromkeys(int(w) for w in labels))
    st = {w: 1 + i for i, w in enumerate(labels)}
    arcs = [(0, st[w], w) for w in labels if first is None or w in first]
    arcs += [(st[a], st[b], int(b)) for a, b in dict.fromkeys((int(a), int(b)) for a, b in allowed_pairs)]
    return 1 + len(labels), arcs, [0] + [int(last is None or w in last) for w in labels]


def grammar_repeat(positions, loop_labels, min_repeat=1):
    """A sequence followed by a loop -- "one command, then any number of digits": word i of a parse is one of the labels
    positions[i], then at least min_repeat words of loop_labels follow, as many as were said.  The parse may end after the
    min_repeat-th looped word and after every one behind it (min_repeat 0: right after the sequence too).  A loop has no
    length: decode it with Engine.decode_onepass_grammar.  Returns (n_states, arcs, final)."""
    n, loop = len(positions), list(dict.fromkeys(int(w) for w in loop_labels))
    arcs = [(i, i + 1, int(w)) for i, ws in enumerate(positions) for w in dict.fromkeys(ws)]
    arcs += [(n + j, n + j + 1, w) for j in range(min_repeat) for w in loop]
    last = n + min_repeat
    arcs += [(last, last, w) for w in loop]
    return last + 1, arcs, [int(s == last) for s in range(last + 1)]


def onepass_grammar_plan(gram, frames_cap=0):
    """sr_onepass_grammar_plan (host only) for a Grammar: dict(row_bytes, rows, block, launches, kept_items, kept_states); rows 0 =
    one row exceeds a launch group's scratch and a call is refused."""
    out = (C.c_uint32 * 6)()
    gram.eng._check(gram.L.sr_onepass_grammar_plan(gram.g, C.c_uint32(frames_cap), out))
    return dict(row_bytes=out[0], rows=out[1], block=out[2], launches=out[3], kept_items=out[4], kept_states=out[5])


def grammar_bigram(labels, cost, first_cost=None, last_cost=None):
    """A weighted word-pair (bigram) grammar: one state per word (1 + its index in labels) plus the start.  cost[a][b] is the
    cost of word b after word a, None = forbidden; first_cost[w] the cost of starting with w, None = forbidden; last_cost[w]
    the final cost after w, None = the parse may not end there.  All three are indexed by label (nested sequences or dicts);
    first_cost / last_cost None: every word may start / end at cost 0.
    Returns (n_states, arcs, final, arc_cost, final_cost) for Engine.grammar()."""
    labels = list(dict.fromkeys(int(w) for w in labels))
    st = {w: 1 + i for i, w in enumerate(labels)}
    arcs, arc_cost = [], []
    for w in labels:
        if first_cost is None or first_cost[w] is not None:
            arcs.append((0, st[w], w))
            arc_cost.append(0 if first_cost is None else int(first_cost[w]))
    for a in labels:
        for b in labels:
            if cost[a][b] is not None:
                arcs.append((st[a], st[b], b))
                arc_cost.append(int(cost[a][b]))
    final = [0] + [int(last_cost is None or last_cost[w] is not None) for w in labels]
    final_cost = [0] + [0 if last_cost is None or last_cost[w] is None else int(last_cost[w]) for w in labels]
    return 1 + len(labels), arcs, final, arc_cost, final_cost


class Grammar:
    """One sr_grammar handle: a word network, with or without costs on its arcs and final states, compiled against its
    engine's store and word map (Engine.grammar).  Setting the templates or the word map again makes it stale: decode calls
    then raise until a new one is compiled."""

    def __init__(self, eng, n_states, arcs, final, arc_cost=None, final_cost=None):
        self.eng, self.L, self.g = eng, eng.L, None
        a = np.zeros(len(arcs), dtype=GRAM_ARC_DTYPE)
        for i, arc in enumerate(arcs):
            a[i] = tuple(arc) + (0,) * (4 - len(arc))
        final = np.ascontiguousarray(final, dtype=np.uint8)
        assert len(final) == n_states
        g = C.c_void_p()
        if arc_cost is None and final_cost is None:
            eng._check(self.L.sr_grammar_create(eng.h, C.c_uint32(n_states), _vp(a), C.c_uint32(len(a)), _vp(final), C.byref(g)))
        else:
            ac = None if arc_cost is None else np.ascontiguousarray(arc_cost, dtype=np.uint32)
            fc = None if final_cost is None else np.ascontiguousarray(final_cost, dtype=np.uint32)
            assert (ac is None or len(ac) == len(a)) and (fc is None or len(fc) == n_states)
            eng._check(self.L.sr_grammar_create_weighted(eng.h, C.c_uint32(n_states), _vp(a), None if ac is None else _vp(ac), C.c_uint32(len(a)),
                                                         _vp(final), None if fc is None else _vp(fc), C.byref(g)))
        self.g, self.n_states = g, n_states

    def plan(self, max_words=8):
        """sr_grammar_plan (host only): dict(row_bytes, rows, launches, from_sets, items_per_level [max_words])."""
        items, out = np.zeros(max_words, np.uint32), (C.c_uint32 * 4)()
        self.eng._check(self.L.sr_grammar_plan(self.g, C.c_uint32(max_words), _vp(items), out))
        return dict(row_bytes=out[0], rows=out[1], launches=out[2], from_sets=out[3], items_per_level=[int(i) for i in items])

    def close(self):
        if getattr(self, "g", None) and getattr(self.eng, "h", None):
            self.L.sr_grammar_destroy(self.g)  # before sr_destroy of its engine
        self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_live_geometry(tpl_rows, K, max_words, utt_frames, chunk_max):
    """Host-only sr_decode_live_geometry: dict(state_bytes on the device per channel, max_tpl_rows that fit, launches one
    feature push enqueues)"""
    L = load_library()
    out = (C.c_uint32 * 3)()
    rc = L.sr_decode_live_geometry(C.c_uint32(tpl_rows), C.c_uint32(K), C.c_uint32(max_words), C.c_uint32(utt_frames), C.c_uint32(chunk_max),
                                   out)
    if rc != 0:
        raise SrError(f"sr_decode_live_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(state_bytes=out[0], max_tpl_rows=out[1], launches=out[2])


class DecodeSession:
    """One sr_decode_live handle (Engine.decode_live): connected-word decoding over chunked features or samples on n_channels
    channels, the decoder's state carried between pushes.  After every push the row of a channel is Engine.decode_words on
    everything pushed to it as one row (include/sr_engine.h, "live connected-word decoding").  GrammarSession shares this body:
    the two C sessions take the same arguments behind their prefix, and sr_gram_live_open one more behind the engine."""

    _PREFIX = "sr_decode_live_"  # the C entry points of the session

    def __init__(self, eng, n_channels, chunk_max, utt_frames, max_words=8, n_words=0, skip_cost=None, word_cost=0, mid=None, _first=()):
        """_first: what the session's open call takes between the engine and n_channels (subclasses)"""
        self.eng, self.L, self.n_channels, self.chunk_max, self.utt_frames = eng, eng.L, n_channels, chunk_max, utt_frames
        self.max_words = max_words
        self._fn("close").restype = None
        self._fn("close").argtypes = [C.c_void_p]
        md = None if mid is None else np.ascontiguousarray(mid, dtype=np.uint32)
        assert md is None or md.shape == (n_channels,)
        self.pcm = md is not None
        self._frames = np.zeros(n_channels, np.uint32)  # what the rows of the pushes said, per channel
        l = C.c_void_p()
        eng._check(self._fn("open")(eng.h, *_first, C.c_uint32(n_channels), C.c_uint32(chunk_max), C.c_uint32(utt_frames),
                                    C.c_uint32(max_words), C.c_uint32(n_words), C.c_uint32(Engine._skip(skip_cost)),
                                    C.c_uint32(word_cost), _vp(md), C.byref(l)))
        self.l = l

    def _fn(self, name):
        return getattr(self.L, self._PREFIX + name)

    def close(self):
        if getattr(self, "l", None):
            self._fn("close")(self.l)
            self.l = None

    def __del__(self):
        try:
            if getattr(self.eng, "h", None):  # a session never outlives its engine's handle
                self.close()
        except Exception:
            pass

    @property
    def frames(self):
        """frames of every channel's recording so far, uint32 [n_channels] (from the rows the calls returned)"""
        return self._frames.copy()

    def _counts(self, counts, width):
        """(host uint32 array or None, n_all, the number of rows a push with these counts emits)"""
        if counts is None:
            return None, width, self.n_channels if width else 0
        ct = np.ascontiguousarray(counts, dtype=np.uint32)
        assert ct.shape == (self.n_channels,)
        return ct, 0, int((ct > 0).sum())

    def _took(self, rows):
        self._frames[rows["channel"]] = rows["frames"]

    def _push_host(self, fn, data, stride, width, counts, max_rows):
        ct, n_all, emit = self._counts(counts, width)
        if max_rows is None:
            max_rows = emit
        W = self.max_words
        rec, words = np.zeros(max_rows, dtype=CHAIN_REC_DTYPE), np.zeros((max_rows, W), dtype=CHAIN_WORD_DTYPE)
        lc = np.zeros((max_rows, W), dtype=np.uint32)
        rows, n = np.zeros(max_rows, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(rec), _vp(words),
                           _vp(lc), _vp(rows), C.byref(n)))
        self._took(rows[:n.value])
        return dict(rec=rec[:n.value], words=words[:n.value], level_cost=lc[:n.value], rows=rows[:n.value], n_rows=n.value)

    def _push_dev(self, fn, data, stride, width, counts, max_rows, level_cost, stream):
        import torch
        ct, n_all, emit = self._counts(counts, width)
        if max_rows is None:
            max_rows = emit
        W, dev = self.max_words, data.device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        cap = max(max_rows, 1)
        rec = torch.empty(cap, 4, dtype=torch.int32, device=dev)[:max_rows]
        words = torch.empty(cap, W, 8, dtype=torch.int32, device=dev)[:max_rows]
        lc = torch.empty(cap, W, dtype=torch.int32, device=dev)[:max_rows] if level_cost else None
        rows, n = np.zeros(max_rows, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(rec), _vp(words),
                           _vp(lc), _vp(rows), C.byref(n), C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            for t in (data, rec, words, lc):
                if t is not None:
                    t.record_stream(stream)  # allocated on the current stream, used on `stream`
        self._took(rows[:n.value])
        return dict(rec=rec[:n.value], words=words[:n.value], level_cost=None if lc is None else lc[:n.value], rows=rows[:n.value],
                    n_rows=n.value)

    def push(self, frames, counts=None, max_rows=None):
        """sr_decode_live_push: frames int16 [n_channels, F, 12], counts [n_channels] (None: F each).  Returns dict(rec
        CHAIN_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE [n_rows, max_words], level_cost uint32 [n_rows, max_words], rows
        CHAIN_LIVE_ROW_DTYPE [n_rows], n_rows) of numpy arrays: one row per channel with a nonzero count."""
        mf = np.ascontiguousarray(frames, dtype=np.int16)
        assert mf.ndim == 3 and mf.shape[0] == self.n_channels and mf.shape[2] == N_COEF
        F = mf.shape[1]
        return self._push_host(self._fn("push"), mf, max(F, 1) * N_COEF, F, counts, max_rows)

    def push_dev(self, frames, counts=None, max_rows=None, level_cost=True, stream=None):
        """sr_decode_live_push_dev on a device tensor: frames int16 [n_channels, F, 12], counts a HOST array [n_channels] (None:
        F each).  Asynchronous on `stream` (a torch.cuda.Stream, or the current one).  Returns dict(rec int32 [n_rows, 4], words
        int32 [n_rows, max_words, 8], level_cost int32 [n_rows, max_words] or None -- device tensors, compact over the emitted
        rows -- rows, n_rows on the host)."""
        import torch
        assert frames.is_cuda and frames.dtype == torch.int16 and frames.is_contiguous()
        assert frames.ndim == 3 and frames.shape[0] == self.n_channels and frames.shape[2] == N_COEF
        F = frames.shape[1]
        return self._push_dev(self._fn("push_dev"), frames, max(F, 1) * N_COEF, F, counts, max_rows, level_cost, stream)

    def push_pcm(self, chunks, counts=None, max_rows=None):
        """sr_decode_live_push_pcm: chunks uint16 [n_channels, S], counts [n_channels] in samples (None: S each); returns as push"""
        pcm = np.ascontiguousarray(chunks, dtype=np.uint16)
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_channels
        S = pcm.shape[1]
        return self._push_host(self._fn("push_pcm"), pcm, max(S, 1), S, counts, max_rows)

    def push_pcm_dev(self, chunks, counts=None, max_rows=None, level_cost=True, stream=None):
        """sr_decode_live_push_pcm_dev: chunks int16 [n_channels, S] on the device (u16 codes, S a multiple of 8); returns as
        push_dev"""
        import torch
        assert chunks.is_cuda and chunks.dtype in (torch.int16, torch.uint16) and chunks.is_contiguous()
        assert chunks.ndim == 2 and chunks.shape[0] == self.n_channels
        S = chunks.shape[1]
        return self._push_dev(self._fn("push_pcm_dev"), chunks, S, S, counts, max_rows, level_cost, stream)

    def end(self, channels):
        """sr_decode_live_end: the listed channels' recordings end here.  Returns dict(rec, words, level_cost, rows, n_rows) as
        push: one row per distinct listed channel, the parse of everything pushed to it; afterwards the channels are as
        freshly opened."""
        ch = np.ascontiguousarray(np.atleast_1d(channels), dtype=np.uint32)
        cap, W = max(len(ch), 1), self.max_words
        rec, words = np.zeros(cap, dtype=CHAIN_REC_DTYPE), np.zeros((cap, W), dtype=CHAIN_WORD_DTYPE)
        lc = np.zeros((cap, W), dtype=np.uint32)
        rows, n = np.zeros(cap, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(self._fn("end")(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(rec), _vp(words), _vp(lc), _vp(rows), C.byref(n)))
        self._frames[rows[:n.value]["channel"]] = 0
        return dict(rec=rec[:n.value], words=words[:n.value], level_cost=lc[:n.value], rows=rows[:n.value], n_rows=n.value)


def onepass_live_geometry(tpl_rows, K, min_tpl_frames, utt_frames, chunk_max, testing=False):
    """Host-only sr_onepass_live_geometry: dict(state_bytes on the device per channel, max_tpl_rows that fit, block = L, launches
    a feature push of chunk_max frames enqueues at most).  testing: the testing library, whose "onepass_block" hook caps the
    blocks."""
    L = load_library(testing)
    out = (C.c_uint32 * 4)()
    rc = L.sr_onepass_live_geometry(C.c_uint32(tpl_rows), C.c_uint32(K), C.c_uint32(min_tpl_frames), C.c_uint32(utt_frames),
                                    C.c_uint32(chunk_max), out)
    if rc != 0:
        raise SrError(f"sr_onepass_live_geometry error {rc}: {L.sr_last_error().decode()}")
    return dict(state_bytes=out[0], max_tpl_rows=out[1], block=out[2], launches=out[3])


class OnePassSession(DecodeSession):
    """One sr_onepass_live handle (Engine.decode_onepass_live): one-pass connected-word decoding over chunked features or
    samples, no word cap.  After every push the row of a channel is Engine.decode_onepass on everything pushed to it as one row
    (include/sr_engine.h, "live one-pass connected-word decoding").  push, push_dev, push_pcm, push_pcm_dev, frames and close
    are DecodeSession's; the rows carry no level costs: dict(rec, words [n_rows, words_cap], rows, n_rows).  commit and
    commit_dev say which words of a channel's parse no later frame can change."""

    _PREFIX = "sr_onepass_live_"

    def __init__(self, eng, n_channels, chunk_max, utt_frames, words_cap, tail=False, skip_cost=None, word_cost=0, mid=None, _first=()):
        """_first: what the session's open call takes between the engine and n_channels (subclasses)"""
        self.eng, self.L, self.n_channels, self.chunk_max, self.utt_frames = eng, eng.L, n_channels, chunk_max, utt_frames
        self.max_words = self.words_cap = words_cap
        self._fn("close").restype = None
        self._fn("close").argtypes = [C.c_void_p]
        md = None if mid is None else np.ascontiguousarray(mid, dtype=np.uint32)
        assert md is None or md.shape == (n_channels,)
        self.pcm = md is not None
        self._frames = np.zeros(n_channels, np.uint32)
        l = C.c_void_p()
        eng._check(self._fn("open")(eng.h, *_first, C.c_uint32(n_channels), C.c_uint32(chunk_max), C.c_uint32(utt_frames), C.c_uint32(words_cap),
                                    C.c_uint32(OP_LIVE_TAIL if tail else 0), C.c_uint32(Engine._skip(skip_cost)), C.c_uint32(word_cost),
                                    _vp(md), C.byref(l)))
        self.l = l

    def _push_host(self, fn, data, stride, width, counts, max_rows):
        ct, n_all, emit = self._counts(counts, width)
        if max_rows is None:
            max_rows = emit
        rec, words = np.zeros(max_rows, dtype=CHAIN_REC_DTYPE), np.zeros((max_rows, self.words_cap), dtype=CHAIN_WORD_DTYPE)
        rows, n = np.zeros(max_rows, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(rec), _vp(words),
                           _vp(rows), C.byref(n)))
        self._took(rows[:n.value])
        return dict(rec=rec[:n.value], words=words[:n.value], rows=rows[:n.value], n_rows=n.value)

    def _push_dev(self, fn, data, stride, width, counts, max_rows, level_cost, stream):
        import torch
        ct, n_all, emit = self._counts(counts, width)
        if max_rows is None:
            max_rows = emit
        W, dev = self.words_cap, data.device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        cap = max(max_rows, 1)
        rec = torch.empty(cap, 4, dtype=torch.int32, device=dev)[:max_rows]
        words = torch.empty(cap, W, 8, dtype=torch.int32, device=dev)[:max_rows]
        rows, n = np.zeros(max_rows, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(fn(self.l, _vp(data), C.c_uint64(stride), _vp(ct), C.c_uint32(n_all), C.c_uint32(max_rows), _vp(rec), _vp(words),
                           _vp(rows), C.byref(n), C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            for t in (data, rec, words):
                t.record_stream(stream)  # allocated on the current stream, used on `stream`
        self._took(rows[:n.value])
        return dict(rec=rec[:n.value], words=words[:n.value], rows=rows[:n.value], n_rows=n.value)

    def end(self, channels):
        """sr_onepass_live_end: the listed channels' recordings end here.  Returns dict(rec, words, rows, n_rows) as push: one
        row per distinct listed channel, the parse of everything pushed to it; afterwards the channels are as freshly opened."""
        ch = np.ascontiguousarray(np.atleast_1d(channels), dtype=np.uint32)
        cap = max(len(ch), 1)
        rec, words = np.zeros(cap, dtype=CHAIN_REC_DTYPE), np.zeros((cap, self.words_cap), dtype=CHAIN_WORD_DTYPE)
        rows, n = np.zeros(cap, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(self._fn("end")(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(rec), _vp(words), _vp(rows), C.byref(n)))
        self._frames[rows[:n.value]["channel"]] = 0
        return dict(rec=rec[:n.value], words=words[:n.value], rows=rows[:n.value], n_rows=n.value)

    def _commit_list(self, channels):
        ch = np.arange(self.n_channels, dtype=np.uint32) if channels is None else np.ascontiguousarray(np.atleast_1d(channels), dtype=np.uint32)
        return ch, max(len(ch), 1)

    def commit(self, channels=None):
        """sr_onepass_live_commit: the words of the listed channels (None: every channel) that no later frame can change.
        Returns dict(crec COMMIT_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE [n_rows, words_cap], rows CHAIN_LIVE_ROW_DTYPE
        [n_rows], n_rows): one row per distinct listed channel; words holds the crec["n_new"] committed words that no earlier
        call delivered, crec["first"] the index of the first of them."""
        ch, cap = self._commit_list(channels)
        crec, words = np.zeros(cap, dtype=COMMIT_REC_DTYPE), np.zeros((cap, self.words_cap), dtype=CHAIN_WORD_DTYPE)
        rows, n = np.zeros(cap, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(self._fn("commit")(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(crec), _vp(words), _vp(rows), C.byref(n)))
        return dict(crec=crec[:n.value], words=words[:n.value], rows=rows[:n.value], n_rows=n.value)

    def commit_dev(self, channels=None, stream=None):
        """sr_onepass_live_commit_dev: as commit(), asynchronous on `stream` (a torch.cuda.Stream, or the current one) behind the
        session's last push.  Returns dict(crec int32 [n_rows, 4], words int32 [n_rows, words_cap, 8] -- device tensors -- rows,
        n_rows on the host)."""
        import torch
        ch, cap = self._commit_list(channels)
        d = self.eng.cfg.device
        dev = torch.device("cuda", d if d >= 0 else torch.cuda.current_device())
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        crec = torch.empty(cap, 4, dtype=torch.int32, device=dev)
        words = torch.empty(cap, self.words_cap, 8, dtype=torch.int32, device=dev)
        rows, n = np.zeros(cap, dtype=CHAIN_LIVE_ROW_DTYPE), C.c_uint32(0)
        self.eng._check(self._fn("commit_dev")(self.l, _vp(ch), C.c_uint32(len(ch)), _vp(crec), _vp(words), _vp(rows), C.byref(n),
                                               C.c_void_p(getattr(stream, "cuda_stream", stream))))
        if isinstance(stream, torch.cuda.Stream):
            for t in (crec, words):
                t.record_stream(stream)  # allocated on the current stream, used on `stream`
        return dict(crec=crec[:n.value], words=words[:n.value], rows=rows[:n.value], n_rows=n.value)


def onepass_grammar_live_geometry(gram, utt_frames, chunk_max):
    """Host-only sr_onepass_gram_live_geometry: dict(state_bytes on the device per channel, max_tpl_rows that fit, block = L,
    launches a feature push of chunk_max frames enqueues, items and states = what the decoder keeps of the grammar)"""
    out = (C.c_uint32 * 6)()
    gram.eng._check(gram.L.sr_onepass_gram_live_geometry(gram.g, C.c_uint32(utt_frames), C.c_uint32(chunk_max), out))
    return dict(state_bytes=out[0], max_tpl_rows=out[1], block=out[2], launches=out[3], items=out[4], states=out[5])


class OnePassGrammarSession(OnePassSession):
    """One sr_onepass_gram_live handle (Engine.decode_onepass_grammar_live): an OnePassSession under a Grammar.  After every
    push the row of a channel is Engine.decode_onepass_grammar on everything pushed to it as one row, the grammar state after
    each word in `reserved` (include/sr_engine.h, "live one-pass grammar decoding").  push, push_dev, push_pcm, push_pcm_dev,
    end, frames, commit and commit_dev are OnePassSession's; set_grammar switches the grammar while every channel is empty.
    commit says which words every parse the recording can still get begins with, also while the row itself is still CH_NONE;
    the state after each word is in `reserved`.  Close the session before its grammar."""

    _PREFIX = "sr_onepass_gram_live_"

    def __init__(self, eng, gram, n_channels, chunk_max, utt_frames, words_cap, tail=False, skip_cost=None, word_cost=0, mid=None):
        super().__init__(eng, n_channels, chunk_max, utt_frames, words_cap, tail, skip_cost, word_cost, mid, _first=(gram.g,))
        self.gram = gram  # kept alive: the session is closed before its grammar

    def _fn(self, name):
        fn = super()._fn(name)
        if name in ("commit", "commit_dev"):  # OnePassSession's methods through _PREFIX: (l, channels, n_ch, crec, cwords, rows, n_rows[, stream])
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * (4 + (name == "commit_dev"))
        return fn

    def set_grammar(self, gram):
        """sr_onepass_gram_live_set_grammar: the grammar of the next dialogue state, or a fresh one in the place of a stale
        one; raises unless every channel is empty (freshly opened or ended)"""
        self.eng._check(self._fn("set_grammar")(self.l, gram.g))
        self.gram = gram


def grammar_live_geometry(gram, max_words, utt_frames, chunk_max):
    """Host-only sr_gram_live_geometry: dict(state_bytes on the device per channel, max_tpl_rows that fit, launches one
    feature push enqueues, columns = the boundary columns per channel: the items kept, summed over the levels)"""
    out = (C.c_uint32 * 4)()
    gram.eng._check(gram.L.sr_gram_live_geometry(gram.g, C.c_uint32(max_words), C.c_uint32(utt_frames), C.c_uint32(chunk_max), out))
    return dict(state_bytes=out[0], max_tpl_rows=out[1], launches=out[2], columns=out[3])


class GrammarSession(DecodeSession):
    """One sr_gram_live handle (Engine.decode_grammar_live): a DecodeSession under a Grammar.  After every push the row of a
    channel is Engine.decode_grammar on everything pushed to it as one row (include/sr_engine.h, "live grammar-constrained
    decoding").  push, push_dev, push_pcm, push_pcm_dev, end, frames and close are DecodeSession's; set_grammar switches the
    grammar while every channel is empty.  Close the session before its grammar."""

    _PREFIX = "sr_gram_live_"

    def __init__(self, eng, gram, n_channels, chunk_max, utt_frames, max_words=8, n_words=0, skip_cost=None, word_cost=0, mid=None):
        super().__init__(eng, n_channels, chunk_max, utt_frames, max_words, n_words, skip_cost, word_cost, mid, _first=(gram.g,))
        self.gram = gram  # kept alive: the session is closed before its grammar

    def set_grammar(self, gram):
        """sr_gram_live_set_grammar: the grammar of the next dialogue state, or a fresh one in the place of a stale one;
        raises unless every channel is empty (freshly opened or ended)"""
        self.eng._check(self._fn("set_grammar")(self.l, gram.g))
        self.gram = gram


def unpack_vad_masks(masks, n_frames=None):
    """Engine.vad_debug_masks' words uint64 [B, 16] as a bool array [B, F]: bit k of word r = frame 63 * r + k (bit 63 of a
    word is never set).  F = n_frames, or all 1 008 frames the words can hold."""
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    assert m.ndim == 2 and m.shape[1] == VAD_MASK_WORDS
    bits = (m[:, :, None] >> np.arange(VAD_MASK_FRAMES, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    out = bits.astype(bool).reshape(m.shape[0], VAD_MASK_WORDS * VAD_MASK_FRAMES)
    return out if n_frames is None else out[:, :n_frames]


def live_segs_from_torch(t):
    """[n, 6] int32 device tensor of sr_live_seg records -> numpy LIVE_SEG_DTYPE array [n]"""
    return t.cpu().numpy().view(np.uint8).reshape(-1, 24).copy().view(LIVE_SEG_DTYPE).reshape(-1)


def pack12(pcm):
    """uint16 [B, S] 12-bit ADC codes -> uint8 [B, ceil(S / 2) * 3]: sample 2i = b[3i] | (b[3i+1] & 0x0F) << 8,
    sample 2i+1 = b[3i+1] >> 4 | b[3i+2] << 4 (the layout sr_recognize_batch_packed12 reads)"""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
    assert pcm.max(initial=0) < 4096, "12-bit codes only"
    B, S = pcm.shape
    if S & 1:
        pcm = np.concatenate([pcm, np.zeros((B, 1), np.uint16)], 1)
    a, b = pcm[:, 0::2].astype(np.uint32), pcm[:, 1::2].astype(np.uint32)
    out = np.empty((B, a.shape[1], 3), np.uint8)
    out[:, :, 0] = a & 0xFF
    out[:, :, 1] = (a >> 8) | ((b & 0xF) << 4)
    out[:, :, 2] = b >> 4
    return out.reshape(B, -1)


def results_from_torch(t):
    """[B,4] int32 device tensor -> numpy structured sr_result array."""
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4).copy().view(RESULT_DTYPE).reshape(-1)


def nbest_from_torch(t):
    """[n, n_best, 4] int32 device tensor -> numpy NBEST_DTYPE array [n, n_best]."""
    a = t.cpu().numpy().view(np.uint32)
    return a.reshape(-1, 4).copy().view(NBEST_DTYPE).reshape(a.shape[:-1])


def vad_from_torch(t):
    return t.cpu().numpy().view(np.uint8).reshape(-1, 48).copy().view(VAD_DTYPE).reshape(-1)


class MultiEngine:
    """sr_multi: ONE process driving several MI355X (utterances sharded, templates replicated, one RCCL all-gather of
    the score matrix).  Mirrors the sr_multi_* section of include/sr_engine.h."""

    def __init__(self, devices, max_frames=119, testing=False, **kw):
        self.L = load_library(testing)
        self.L.sr_multi_num_devices.restype = C.c_uint32
        cfg = Config()
        self.L.sr_default_config(C.byref(cfg))
        cfg.max_frames = max_frames
        for k, v in kw.items():
            setattr(cfg, k, v)
        self.cfg, self.max_frames = cfg, max_frames
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        self._check(self.L.sr_multi_create(C.byref(cfg), devs, C.c_uint32(len(devices)), C.byref(h)))
        self.h, self.devices, self.K = h, list(devices), 0

    def _check(self, rc):
        if rc != 0:
            raise SrError(f"sr_multi error {rc}: {self.L.sr_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.L.sr_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_templates_dense(self, mfcc, frames, valid=None):
        mfcc = np.ascontiguousarray(mfcc, dtype=np.int16)
        frames = np.ascontiguousarray(frames, dtype=np.uint32)
        K = mfcc.shape[0]
        valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        self._check(self.L.sr_multi_set_templates_dense(self.h, _vp(mfcc), _vp(frames), _vp(valid), C.c_uint32(K),
                                                        C.c_uint32(mfcc.shape[1] * mfcc.shape[2])))
        self.K = K

    def set_templates_store(self, store, stride=4096):
        store = np.ascontiguousarray(store, dtype=np.uint8)
        self._check(self.L.sr_multi_set_templates(self.h, _vp(store), C.c_uint32(len(store) // stride), C.c_uint32(stride)))
        self.K = len(store) // stride

    def recognize(self, pcm):
        """pcm uint16 [B, S] on the host -> (results [B], gathered scores [B, K])"""
        pcm = np.ascontiguousarray(pcm, dtype=np.uint16)
        B, S = pcm.shape
        res = np.zeros(B, dtype=RESULT_DTYPE)
        sc = np.zeros((B, self.K), dtype=np.uint32)
        self._check(self.L.sr_multi_recognize(self.h, _vp(pcm), C.c_uint64(S), C.c_uint32(S), C.c_uint32(B), _vp(res), _vp(sc)))
        return res, sc

    def engine(self, i):
        """the sr_engine of devices[i] (sr_multi_engine), as a borrowed Engine: profiling hooks, stage-level calls"""
        self.L.sr_multi_engine.restype = C.c_void_p
        h = self.L.sr_multi_engine(self.h, C.c_uint32(i))
        if not h:
            raise SrError(f"sr_multi_engine({i}): no such device")
        cfg = Config.from_buffer_copy(self.cfg)
        cfg.device = self.devices[i]
        return Engine.borrowed(h, cfg, self.max_frames, self.L)

    def recognize_dev(self, pcm_list, results_list, scores_all_list, buf_len=None, streams=None):
        """device-resident shards: torch tensors per device (pcm int16/uint16 [Bp, S], results int32 [Bp, 4],
        scores_all int32 [n_dev*Bp, K]).  streams = None: the handle's own streams, returns when they have drained;
        streams = one torch.cuda.Stream per device: asynchronous on those streams."""
        n = len(self.devices)
        Bp, S = pcm_list[0].shape
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        st = None if streams is None else (C.c_void_p * n)(*[s.cuda_stream for s in streams])
        self._check(self.L.sr_multi_recognize_dev(self.h, arr(pcm_list), C.c_uint64(pcm_list[0].stride(0)),
                                                  C.c_uint32(S if buf_len is None else buf_len), C.c_uint32(Bp),
                                                  arr(results_list), arr(scores_all_list), st))
