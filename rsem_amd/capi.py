"""ctypes binding of librsem_hip.so (include/rsem_hip.h).  No fallbacks: a missing library raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSEM_HIP_LIB: another build of the same library (tuning experiments build variants next to it: tools/build_variants.sh)
LIB_PATH = os.environ.get("RSEM_HIP_LIB") or os.path.join(_HERE, "librsem_hip.so")

KERNEL_AUTO, KERNEL_CSR, KERNEL_SELL, KERNEL_LANE = 0, 1, 2, 3
GIBBS_EXACT, GIBBS_PARALLEL = 0, 1
GIBBS_ORDER_LONG = 255  # RSEM_GIBBS_ORDER_LONG

_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")


class RsemHipError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__("librsem_hip: status %d (%s): %s" % (status, _strerror(status), detail))
        self.status = status


ABI_VERSION = 4  # rsem_hip_abi_version() of the include/rsem_hip.h these bindings were written against


class CiProfile(C.Structure):
    _fields_ = [("sample_ms", C.c_double), ("sort_ms", C.c_double), ("interval_ms", C.c_double), ("total_ms", C.c_double),
                ("n_draws", C.c_uint64), ("n_keys_sorted", C.c_uint64)]


class GibbsProfile(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("sweep_ms", C.c_double), ("sweeps", C.c_int64), ("chains", C.c_int32), ("team", C.c_int32), ("reduce_ms", C.c_double)]


class GibbsDiagSummary(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("sequences", C.c_int32), ("n_defined", C.c_int32), ("max_rhat_id", C.c_int32),
                ("min_ess_id", C.c_int32), ("n_rhat_gt_1p01", C.c_int32), ("n_rhat_gt_1p1", C.c_int32), ("n_long", C.c_int32),
                ("max_rhat", C.c_double), ("min_ess", C.c_double), ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class KmerInfo(C.Structure):
    _fields_ = [("n_kmers", C.c_uint64), ("n_groups", C.c_uint64), ("n_batches", C.c_int32), ("n_chunks", C.c_int32),
                ("batch_items", C.c_uint64), ("max_batch_items", C.c_uint64), ("batch_bytes", C.c_uint64),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class DepthInfo(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_tiles_touched", C.c_uint64), ("n_batches", C.c_int32), ("n_launches", C.c_int32),
                ("batch_items", C.c_uint64), ("device_bytes", C.c_uint64), ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class GmapInfo(C.Structure):
    _fields_ = [("n_groups", C.c_uint64), ("n_alignments_in", C.c_uint64), ("n_alignments_out", C.c_uint64), ("n_cigar_words", C.c_uint64),
                ("n_batches", C.c_int32), ("n_launches", C.c_int32), ("batch_items", C.c_uint64), ("device_bytes", C.c_uint64),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class RefseqInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("raw_bytes", C.c_uint64), ("n_bases", C.c_uint64), ("n_segments", C.c_uint64),
                ("gathered_bytes", C.c_uint64), ("n_batches", C.c_int32), ("n_launches", C.c_int32), ("batch_bytes", C.c_uint64),
                ("store_pad", C.c_uint64), ("device_bytes", C.c_uint64), ("upload_ms", C.c_double), ("kernel_ms", C.c_double),
                ("download_ms", C.c_double)]


class AlncheckVerdict(C.Structure):
    _fields_ = [("code", C.c_int32), ("mate", C.c_int32), ("unit_record", C.c_int64), ("units_ok", C.c_uint64), ("cigar_op", C.c_uint32), ("paired", C.c_int32),
                ("n_records", C.c_uint64), ("n_units", C.c_uint64), ("n_groups", C.c_uint64), ("resident_groups", C.c_uint64), ("resident_name_bytes", C.c_uint64),
                ("n_batches", C.c_int32), ("n_launches", C.c_int32), ("batch_items", C.c_uint64), ("device_bytes", C.c_uint64),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class AlncheckInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_groups", C.c_uint64), ("n_kept", C.c_uint64), ("n_batches", C.c_int32), ("n_launches", C.c_int32),
                ("batch_items", C.c_uint64), ("device_bytes", C.c_uint64), ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class PairscanVerdict(C.Structure):
    _fields_ = [("code", C.c_int32), ("n_batches", C.c_int32), ("group", C.c_int64), ("group_record", C.c_int64), ("n_records", C.c_uint64), ("n_groups", C.c_uint64),
                ("n_sorted_groups", C.c_uint64), ("n_launches", C.c_int32), ("reserved", C.c_int32), ("batch_items", C.c_uint64), ("device_bytes", C.c_uint64),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class SimModel(C.Structure):
    _fields_ = [("type", C.c_int32), ("M", C.c_int32), ("has_mld", C.c_int32), ("est_rspd", C.c_int32), ("B", C.c_int32), ("pro_len", C.c_int32), ("g_lb", C.c_int32),
                ("g_ub", C.c_int32), ("m_lb", C.c_int32), ("m_ub", C.c_int32), ("prob_f", C.c_double)] + [
        (n, C.c_void_p) for n in ("theta_cdf", "full_len", "tot_len", "seq_off", "seq", "g_cdf", "m_cdf", "r_pdf", "r_cdf", "qc_init", "qc_trans", "pc", "npc")]


class SimBatch(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("stride", C.c_int32), ("status", C.c_int32), ("n_reads", C.c_int64), ("resimulations", C.c_uint64)] + [
        (n, C.c_void_p) for n in ("sid", "dir", "pos", "insert_l", "len1", "len2", "attempts", "seq1", "qual1", "seq2", "qual2")] + [
        ("n_chunks", C.c_int32), ("n_launches", C.c_int32), ("stream_words", C.c_uint64), ("device_bytes", C.c_uint64), ("words_ms", C.c_double),
        ("upload_ms", C.c_double), ("search_ms", C.c_double), ("body_ms", C.c_double), ("download_ms", C.c_double)]


class SimKnobs(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("batch_reads", "chunk_words", "tile", "attempt_cap", "lds_tables")]


class EmProfile(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("estep_ms_sum", C.c_double), ("estep_launches", C.c_int32),
                ("rounds", C.c_int32), ("algorithmic_bytes_per_round", C.c_uint64)]


PROGRESS_FN = C.CFUNCTYPE(None, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -m rsem_amd.build` (hipcc, gfx950). "
                              "There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        vp, i32, u64, dbl, ci = C.c_void_p, C.c_int32, C.c_uint64, C.c_double, C.c_int
        L.rsem_hip_strerror.restype = C.c_char_p
        L.rsem_hip_strerror.argtypes = [ci]
        L.rsem_hip_last_error.restype = C.c_char_p
        L.rsem_hip_device_count.argtypes = [C.POINTER(ci)]
        L.rsem_hip_device_info.argtypes = [ci, C.c_char_p, C.POINTER(C.c_int64)]
        L.rsem_hip_abi_version.restype = ci
        if L.rsem_hip_abi_version() != ABI_VERSION:  # the ctypes structures below mirror ONE layout of include/rsem_hip.h
            raise ImportError("%s speaks ABI %d, rsem_amd/capi.py expects %d: rebuild it (`python -m rsem_amd.build --force`)"
                              % (LIB_PATH, L.rsem_hip_abi_version(), ABI_VERSION))
        L.rsem_hip_stream_probe.argtypes = [ci, u64, ci, C.POINTER(dbl), C.POINTER(dbl)]
        L.rsem_em_create.argtypes = [C.POINTER(vp), ci, i32, u64, u64, _u64p, vp, vp, vp]
        L.rsem_em_set_values.argtypes = [vp, _f64p, _f64p]
        L.rsem_em_get_values.argtypes = [vp, _f64p, _f64p]
        L.rsem_em_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.rsem_em_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
        L.rsem_em_debug_trace.argtypes = [vp, _f64p, vp, C.POINTER(C.c_uint32)]
        L.rsem_em_debug_far.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)] + [vp] * 6
        L.rsem_em_destroy.argtypes = [vp]
        L.rsem_em_set_comm.argtypes = [vp, vp]
        L.rsem_em_set_progress.argtypes = [vp, vp, vp]
        L.rsem_em_shard_rows.argtypes = [u64, _u64p, ci, _u64p]
        L.rsem_em_step.argtypes = [vp, _f64p, dbl, vp, vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(i32)]
        L.rsem_em_run.argtypes = [vp, _f64p, dbl, ci, ci, ci, C.POINTER(ci), vp, C.POINTER(dbl), C.POINTER(i32), vp]
        L.rsem_em_expected_weights.argtypes = [vp, _f64p, dbl, vp, vp, vp]
        L.rsem_gibbs_create.argtypes = [C.POINTER(vp), ci, i32, u64, u64, _u64p, _i32p, _f64p, _i32p, vp, dbl, dbl, u64,
                                        _f64p, _f64p, i32, _i32p]
        L.rsem_gibbs_run.argtypes = [vp, ci, C.c_uint32, ci, ci, ci, ci, vp, _f64p, _f64p, _f64p, _f64p, _f64p, vp]
        L.rsem_gibbs_run_chains.argtypes = [vp, ci, ci, _u32p, ci, _i32p, ci, ci, vp, _f64p, _f64p, _f64p, _f64p, _f64p, vp, vp]
        L.rsem_gibbs_set_comm.argtypes = [vp, vp]
        L.rsem_gibbs_set_allele_groups.argtypes = [vp, i32, _i32p]
        L.rsem_gibbs_get_pve_c_trans.argtypes = [vp, _f64p]
        L.rsem_gibbs_debug_order.argtypes = [vp, _u32p, _u8p, C.POINTER(C.c_uint32)]
        L.rsem_gibbs_debug_units.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp]
        L.rsem_gibbs_debug_unit_windows.argtypes = [vp, C.POINTER(C.c_uint32), vp]
        L.rsem_gibbs_destroy.argtypes = [vp]
        L.rsem_comm_unique_id.argtypes = [C.c_char_p]
        L.rsem_comm_create.argtypes = [C.POINTER(vp), ci, ci, ci, C.c_char_p]
        L.rsem_comm_create_local.argtypes = [C.POINTER(vp), ci, C.POINTER(ci)]
        L.rsem_comm_rank.argtypes = [vp]
        L.rsem_comm_world.argtypes = [vp]
        L.rsem_comm_allreduce_f64.argtypes = [vp, vp, u64, vp]
        L.rsem_comm_destroy.argtypes = [vp]
        L.rsem_gibbs_chain_seeds.argtypes = [C.c_uint32, ci, _u32p]
        L.rsem_gibbs_diagnose.argtypes = [ci, i32, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.rsem_ci_calculate.argtypes = [ci, i32, i32, i32, _i32p, _f64p, _f64p, dbl, u64, dbl, i32, _i32p, i32, vp,
                                        _f32p, _f32p, _f32p, _f32p, vp, vp, vp]
        L.rsem_ci_calculate_samples.argtypes = [ci, i32, i32, _f32p, _f32p, dbl, i32, _i32p, i32, vp,
                                                _f32p, _f32p, _f32p, _f32p, vp, vp, vp]
        L.rsem_ci_sample.argtypes = [ci, i32, i32, i32, _i32p, _f64p, _f64p, dbl, u64, _f32p, _f32p]
        L.rsem_ci_intervals.argtypes = [ci, C.c_int64, i32, _f32p, dbl, _f32p, _f32p, _f32p]
        L.rsem_kmer_shared_counts.argtypes = [ci, i32, _u64p, vp, i32, _u32p, vp]
        L.rsem_depth_accumulate.argtypes = [ci, u64, u64, vp, vp, vp, vp, vp]
        L.rsem_gmap_create.argtypes = [C.POINTER(vp), ci, i32, vp, vp, vp, vp, vp, vp]
        L.rsem_gmap_convert.argtypes = [vp, i32, C.c_int64, C.c_int64] + [vp] * 14 + [u64, vp, vp, vp]
        L.rsem_gmap_destroy.argtypes = [vp]
        L.rsem_gmap_destroy.restype = None
        L.rsem_refseq_create.argtypes = [C.POINTER(vp), ci, u64]
        L.rsem_refseq_load.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64), vp, vp]
        L.rsem_refseq_gather.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
        L.rsem_refseq_download.argtypes = [vp, u64, u64, vp]
        L.rsem_refseq_get_info.argtypes = [vp, vp]
        L.rsem_refseq_destroy.argtypes = [vp]
        L.rsem_refseq_destroy.restype = None
        L.rsem_alncheck_create.argtypes = [C.POINTER(vp), ci, i32, vp]
        L.rsem_alncheck_push.argtypes = [vp, C.c_int64] + [vp] * 9 + [i32, vp]
        L.rsem_alncheck_destroy.argtypes = [vp]
        L.rsem_alncheck_destroy.restype = None
        L.rsem_alncheck_unique.argtypes = [ci, C.c_int64, vp, vp, vp, vp, vp]
        L.rsem_pairscan_create.argtypes = [C.POINTER(vp), ci]
        L.rsem_pairscan_reorder.argtypes = [vp, C.c_int64] + [vp] * 6 + [i32, vp, vp]
        L.rsem_pairscan_destroy.argtypes = [vp]
        L.rsem_pairscan_destroy.restype = None
        L.rsem_sim_read_knobs.argtypes = [vp]
        L.rsem_sim_create.argtypes = [C.POINTER(vp), vp, ci]
        L.rsem_sim_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        L.rsem_sim_counter_batch.argtypes = [vp, u64, u64, C.c_int64, vp]
        L.rsem_sim_reference_begin.argtypes = [vp, C.c_uint32]
        L.rsem_sim_reference_batch.argtypes = [vp, C.c_int64, vp]
        L.rsem_sim_totals.argtypes = [vp, _u64p, C.POINTER(u64)]
        L.rsem_sim_destroy.argtypes = [vp]
        L.rsem_sim_destroy.restype = None
        _lib = L
    return _lib


def _strerror(status):
    return lib().rsem_hip_strerror(status).decode()


def _check(status):
    if status != 0:
        raise RsemHipError(status, lib().rsem_hip_last_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    _check(lib().rsem_hip_device_count(C.byref(n)))
    return n.value


def stream_probe(device=0, nbytes=4 << 30, reps=5):
    """Measured device STREAM rates in GB/s: (read-only, copy with read + write bytes counted)."""
    r, c = C.c_double(), C.c_double()
    _check(lib().rsem_hip_stream_probe(device, int(nbytes), int(reps), C.byref(r), C.byref(c)))
    return r.value, c.value


class EmContext:
    """One GPU's EM shard (rsem_em_ctx).  Mirrors E_STEP<> / EM<> of EM.cpp for frozen CSR values."""

    def __init__(self, M, row_ptr, sid, conprb=None, ncp=None, device=0):
        self.M = int(M)
        self.N1 = len(row_ptr) - 1
        self.nnz = len(sid)
        row_ptr = np.ascontiguousarray(row_ptr, np.uint64)
        sid = np.ascontiguousarray(sid, np.int32)
        if conprb is not None:
            conprb = np.ascontiguousarray(conprb, np.float64)
            ncp = np.ascontiguousarray(ncp, np.float64)
        self._h = C.c_void_p()
        _check(lib().rsem_em_create(C.byref(self._h), device, self.M, self.N1, self.nnz, row_ptr, _ptr(sid), _ptr(conprb),
                                    _ptr(ncp)))

    def close(self):
        if self._h:
            lib().rsem_em_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_values(self, conprb, ncp):
        _check(lib().rsem_em_set_values(self._h, np.ascontiguousarray(conprb, np.float64),
                                        np.ascontiguousarray(ncp, np.float64)))

    def set_option(self, key, value):
        _check(lib().rsem_em_set_option(self._h, key.encode(), int(value)))

    def info(self, key):
        v = C.c_int64()
        _check(lib().rsem_em_get_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def get_values(self):
        cp, ncp = np.zeros(self.nnz), np.zeros(self.N1)
        _check(lib().rsem_em_get_values(self._h, cp, ncp))
        return cp, ncp

    def set_comm(self, comm):
        _check(lib().rsem_em_set_comm(self._h, comm._h if comm is not None else None))

    def set_progress(self, fn):
        """fn(round, sum, bChange, totNum) for every round of run() (EM.cpp:415), or None."""
        self._cb = PROGRESS_FN(lambda r, s, b, t, u: fn(r, s, b, t)) if fn else None
        _check(lib().rsem_em_set_progress(self._h, C.cast(self._cb, C.c_void_p) if fn else None, None))

    def step(self, theta, N0):
        theta = np.ascontiguousarray(theta, np.float64)
        counts, theta_new = np.zeros(self.M + 1), np.zeros(self.M + 1)
        s, b, t = C.c_double(), C.c_double(), C.c_int32()
        _check(lib().rsem_em_step(self._h, theta, float(N0), _ptr(counts), _ptr(theta_new), C.byref(s), C.byref(b),
                                  C.byref(t)))
        return counts, theta_new, s.value, b.value, t.value

    def run(self, theta, N0, round0=0, min_round=20, max_round=10000, profile=False):
        theta = np.array(theta, np.float64)
        counts = np.zeros(self.M + 1)
        r, b, t = C.c_int(), C.c_double(), C.c_int32()
        prof = EmProfile() if profile else None
        _check(lib().rsem_em_run(self._h, theta, float(N0), round0, min_round, max_round, C.byref(r), _ptr(counts),
                                 C.byref(b), C.byref(t), C.cast(C.pointer(prof), C.c_void_p) if profile else None))
        out = dict(theta=theta, rounds=r.value, counts=counts, bChange=b.value, totNum=t.value)
        if profile:
            out["profile"] = prof
        return out

    def debug_trace(self, theta):
        """Per-workgroup (start, end) timestamps of one traced E-step launch, a row per unit in dispatch order."""
        t = np.zeros((max(self.info("units"), 1), 2), np.uint64)
        n = C.c_uint32(len(t))
        _check(lib().rsem_em_debug_trace(self._h, np.ascontiguousarray(theta, np.float64), _ptr(t), C.byref(n)))
        return t[:n.value]

    def debug_far(self):
        """rsem_em_debug_far: the split rows' far entries in row order (far_ptr[n_x_slots + 1] by row slot - x_slot_base, far_sid,
        far_src = index into the caller's arrays) and in column order (csc_sid, csc_slot, csc_src); every size 0 without split rows."""
        base, nxs, nf = C.c_uint32(), C.c_uint32(0), C.c_uint64(0)
        _check(lib().rsem_em_debug_far(self._h, C.byref(base), C.byref(nxs), C.byref(nf), *([None] * 6)))
        n = max(nf.value, 1)  # (an empty numpy array may have no address to give)
        out = dict(far_ptr=np.zeros(nxs.value + 1, np.uint64), far_sid=np.zeros(n, np.int32), far_src=np.zeros(n, np.uint64),
                   csc_sid=np.zeros(n, np.int32), csc_slot=np.zeros(n, np.uint32), csc_src=np.zeros(n, np.uint64))
        _check(lib().rsem_em_debug_far(self._h, C.byref(base), C.byref(nxs), C.byref(nf), *[_ptr(a) for a in out.values()]))
        out = {k: (a if k == "far_ptr" else a[:nf.value]) for k, a in out.items()}
        out.update(x_slot_base=int(base.value), n_x_slots=int(nxs.value), n_far=int(nf.value))
        return out

    def expected_weights(self, theta, N0, want_weights=True):
        theta = np.ascontiguousarray(theta, np.float64)
        counts = np.zeros(self.M + 1)
        w = np.zeros(self.nnz) if want_weights else None
        wn = np.zeros(self.N1) if want_weights else None
        _check(lib().rsem_em_expected_weights(self._h, theta, float(N0), _ptr(counts), _ptr(w), _ptr(wn)))
        return counts, w, wn


class GibbsContext:
    """One GPU's Gibbs sampler state (rsem_gibbs_ctx).  Mirrors Gibbs() of Gibbs.cpp."""

    def __init__(self, M, row_ptr, sid, conprb, init_counts, alpha, pseudoC, totc, N0, eel, mw, grp, device=0):
        self.M = int(M)
        self.m = len(grp) - 1
        self.N1 = len(row_ptr) - 1
        self._h = C.c_void_p()
        alpha = None if alpha is None else np.ascontiguousarray(alpha, np.float64)
        _check(lib().rsem_gibbs_create(C.byref(self._h), device, self.M, len(row_ptr) - 1, len(sid),
                                       np.ascontiguousarray(row_ptr, np.uint64), np.ascontiguousarray(sid, np.int32),
                                       np.ascontiguousarray(conprb, np.float64),
                                       np.ascontiguousarray(init_counts, np.int32), _ptr(alpha), float(pseudoC),
                                       float(totc), int(N0), np.ascontiguousarray(eel, np.float64),
                                       np.ascontiguousarray(mw, np.float64), self.m, np.ascontiguousarray(grp, np.int32)))

    def close(self):
        if self._h:
            lib().rsem_gibbs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, mode, seed, burnin, nsamples, gap, thin=1, want_vectors=True):
        cv = np.zeros((nsamples, self.M + 1), np.int32) if want_vectors else None
        acc = [np.zeros(self.M + 1) for _ in range(4)] + [np.zeros(self.m)]
        ms = C.c_double()
        _check(lib().rsem_gibbs_run(self._h, mode, int(seed), burnin, nsamples, gap, thin, _ptr(cv), *acc,
                                    C.cast(C.pointer(ms), C.c_void_p)))
        return cv, acc, ms.value

    def set_comm(self, comm):
        _check(lib().rsem_gibbs_set_comm(self._h, comm._h if comm is not None else None))

    def debug_order(self):
        """rsem_gibbs_debug_order: (order, lg, n_sell_rows) of the PARALLEL sampler's layout -- order[p] = the caller's read at
        sorted position p (the key of its random number), lg[p] = log2 of its lanes, GIBBS_ORDER_LONG for the reads that stay
        in the CSR (positions n_sell_rows and up)."""
        order, lg = np.zeros(self.N1, np.uint32), np.zeros(self.N1, np.uint8)
        n_sell = C.c_uint32()
        _check(lib().rsem_gibbs_debug_order(self._h, order, lg, C.byref(n_sell)))
        return order, lg, int(n_sell.value)

    def debug_units(self):
        """rsem_gibbs_debug_units: (T, units) -- units[u] = (first slice within the shape, slices, slices per wave, far flag, lg, K)."""
        T, n = C.c_uint32(), C.c_uint32(0)
        _check(lib().rsem_gibbs_debug_units(self._h, C.byref(T), C.byref(n), None))
        out = np.zeros((n.value, 6), np.uint32)
        _check(lib().rsem_gibbs_debug_units(self._h, C.byref(T), C.byref(n), out.ctypes.data))
        return int(T.value), out

    def debug_unit_windows(self):
        """rsem_gibbs_debug_unit_windows: windows[u] = (first id, ids) of the LDS window of unit u of debug_units()."""
        n = C.c_uint32(0)
        _check(lib().rsem_gibbs_debug_unit_windows(self._h, C.byref(n), None))
        out = np.zeros((n.value, 2), np.int32)
        _check(lib().rsem_gibbs_debug_unit_windows(self._h, C.byref(n), out.ctypes.data))
        return out

    def set_allele_groups(self, ta):
        ta = np.ascontiguousarray(ta, np.int32)
        _check(lib().rsem_gibbs_set_allele_groups(self._h, len(ta) - 1, ta))
        self.m_trans = len(ta) - 1

    def get_pve_c_trans(self):
        """rsem_gibbs_get_pve_c_trans: the last run's squared per-transcript (over alleles) count sums; RSEM_ERR_STATE when
        allele groups were never set or no chain has run since."""
        out = np.zeros(max(getattr(self, "m_trans", 0), 1))
        _check(lib().rsem_gibbs_get_pve_c_trans(self._h, out))
        return out[:getattr(self, "m_trans", 0)]

    def run_chains(self, mode, seeds, burnin, nsamples, gap, thin=1, want_vectors=True):
        """rsem_gibbs_run_chains: all chains of this GPU in one call.  Returns (list of count-vector arrays or None,
        [pme_c, pve_c, pme_tpm, pme_fpkm, pve_c_genes] summed over the chains, pve_c_trans or None, GibbsProfile)."""
        seeds = np.ascontiguousarray(seeds, np.uint32)
        ns = np.ascontiguousarray(nsamples, np.int32)
        n = len(seeds)
        assert len(ns) == n
        cvs, ptrs = None, None
        if want_vectors:
            cvs = [np.zeros((int(k), self.M + 1), np.int32) for k in ns]
            ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in cvs])
        acc = [np.zeros(self.M + 1) for _ in range(4)] + [np.zeros(self.m)]
        mt = getattr(self, "m_trans", 0)
        trans = np.zeros(mt) if mt else None
        prof = GibbsProfile()
        _check(lib().rsem_gibbs_run_chains(self._h, mode, n, seeds, burnin, ns, gap, thin, ptrs, *acc, _ptr(trans),
                                           C.cast(C.pointer(prof), C.c_void_p)))
        return cvs, acc, trans, prof


COMM_ID_BYTES = 128


class Comm:
    """rsem_comm: one rank of a communicator (RCCL, or the same-process LOCAL kind)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(lib().rsem_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def create(cls, device, rank, world, uid):
        h = C.c_void_p()
        _check(lib().rsem_comm_create(C.byref(h), device, rank, world, uid))
        return cls(h)

    @classmethod
    def create_local(cls, devices):
        n = len(devices)
        hs = (C.c_void_p * n)()
        _check(lib().rsem_comm_create_local(hs, n, (C.c_int * n)(*devices)))
        return [cls(C.c_void_p(h)) for h in hs]

    @property
    def rank(self):
        return lib().rsem_comm_rank(self._h)

    @property
    def world(self):
        return lib().rsem_comm_world(self._h)

    def allreduce(self, d_ptr, n, stream=0):
        _check(lib().rsem_comm_allreduce_f64(self._h, d_ptr, n, stream))

    def close(self):
        if self._h:
            lib().rsem_comm_destroy(self._h)
            self._h = C.c_void_p()


def em_shard_rows(row_ptr, world):
    """rsem_em_shard_rows: the reference's split of the reads over `world` workers (EM.cpp:135-157)."""
    rp = np.ascontiguousarray(row_ptr, np.uint64)
    out = np.zeros(world + 1, np.uint64)
    _check(lib().rsem_em_shard_rows(len(rp) - 1, rp, world, out))
    return [int(x) for x in out]


def gibbs_chain_seeds(seed, n):
    out = np.zeros(n, np.uint32)
    _check(lib().rsem_gibbs_chain_seeds(int(seed), n, out))
    return out


def gibbs_diagnose(cvs, device=0):
    """rsem_gibbs_diagnose: split-R-hat and effective sample size of a run's count vectors.  cvs: one (nsamples[k], M+1) int32 array
    per chain, as GibbsContext.run_chains returns them.  Returns (mean, sd, rhat, ess, lag, summary dict), arrays of M+1."""
    cvs = [np.ascontiguousarray(a, np.int32) for a in cvs]
    n = len(cvs)
    M1 = cvs[0].shape[1] if n else 1
    assert all(a.ndim == 2 and a.shape[1] == M1 for a in cvs)
    ns = np.array([a.shape[0] for a in cvs], np.int32)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in cvs])
    mean, sd, rhat, ess = (np.zeros(M1) for _ in range(4))
    lag = np.zeros(M1, np.int32)
    sm = GibbsDiagSummary()
    _check(lib().rsem_gibbs_diagnose(device, M1 - 1, n, _ptr(ns), C.cast(ptrs, C.c_void_p), _ptr(mean), _ptr(sd), _ptr(rhat), _ptr(ess),
                                     _ptr(lag), C.addressof(sm)))
    return mean, sd, rhat, ess, lag, {k: getattr(sm, k) for k, _ in GibbsDiagSummary._fields_}


def kmer_shared_counts(seq_off, codes, k, device=0):
    """rsem_kmer_shared_counts: per transcript the number of k-mer start positions whose k-mer also occurs in another transcript.
    codes: uint8 0 .. 4 (A C G T N), transcript t = codes[seq_off[t]:seq_off[t+1]].  Returns (shared uint32[M], info dict)."""
    seq_off = np.ascontiguousarray(seq_off, np.uint64)
    codes = np.ascontiguousarray(codes, np.uint8)
    M = len(seq_off) - 1
    assert M >= 0 and (M == 0 or int(seq_off[-1]) <= codes.size)
    shared = np.zeros(max(M, 1), np.uint32)
    info = KmerInfo()
    _check(lib().rsem_kmer_shared_counts(device, M, seq_off, _ptr(codes), int(k), shared, C.addressof(info)))
    return shared[:M], {f: getattr(info, f) for f, _ in KmerInfo._fields_}


def depth_accumulate(n_bases, start, length, w, depth=None, device=0):
    """rsem_depth_accumulate: depth[b] = the fold, in block order, of w[i] over the blocks [start[i], start[i] + length[i]) that cover
    base b, continued from `depth` (zeros where None).  Returns (depth float64[n_bases], info dict); `depth` itself is not changed."""
    start = np.ascontiguousarray(start, np.uint64)
    length = np.ascontiguousarray(length, np.uint32)
    w = np.ascontiguousarray(w, np.float64)
    assert start.shape == length.shape == w.shape and start.ndim == 1
    out = np.zeros(int(n_bases), np.float64) if depth is None else np.array(depth, np.float64, order="C")
    assert out.shape == (int(n_bases),)
    info = DepthInfo()
    _check(lib().rsem_depth_accumulate(device, int(n_bases), len(start), _ptr(start), _ptr(length), _ptr(w), _ptr(out), C.addressof(info)))
    return out, {f: getattr(info, f) for f, _ in DepthInfo._fields_}


def ci_intervals(rows, confidence, device=0):
    """calcCI (calcCI.cpp:216-284) for every row of a (nrows, nSamples) float32 array -> lb, ub, cqv."""
    rows = np.ascontiguousarray(rows, np.float32)
    n, ns = rows.shape
    lb, ub, cqv = (np.zeros(n, np.float32) for _ in range(3))
    _check(lib().rsem_ci_intervals(device, n, ns, rows, float(confidence), lb, ub, cqv))
    return lb, ub, cqv


def ci_sample(cvecs, nSpC, eel, mw, pseudoC=1.0, seed=0, device=0):
    """Phase I of calcCI.cpp alone: (M, nCV*nSpC) float32 TPM samples and l_bars."""
    cvecs = np.ascontiguousarray(cvecs, np.int32)
    nCV, M1 = cvecs.shape
    M = M1 - 1
    tpm = np.zeros((M, nCV * nSpC), np.float32)
    lbar = np.zeros(nCV * nSpC, np.float32)
    _check(lib().rsem_ci_sample(device, M, nCV, nSpC, cvecs, np.ascontiguousarray(eel, np.float64),
                                np.ascontiguousarray(mw, np.float64), float(pseudoC), int(seed), tpm, lbar))
    return tpm, lbar


def _ci_outputs(M, gene_starts, trans_starts):
    gs = np.ascontiguousarray(gene_starts, np.int32)
    m = len(gs) - 1
    out = {k: np.zeros((3, n), np.float32) for k, n in (("tpm", M), ("fpkm", M), ("gene_tpm", m), ("gene_fpkm", m))}
    ts = None
    mt = 0
    if trans_starts is not None:
        ts = np.ascontiguousarray(trans_starts, np.int32)
        mt = len(ts) - 1
        out["iso_tpm"] = np.zeros((3, mt), np.float32)
        out["iso_fpkm"] = np.zeros((3, mt), np.float32)
    return out, gs, m, ts, mt


def ci_calculate(cvecs, nSpC, eel, mw, gene_starts, confidence=0.95, pseudoC=1.0, seed=0, trans_starts=None, device=0):
    """rsem-calculate-credibility-intervals in one call.  Returns a dict of (3, n) float32 arrays [lb, ub, cqv]:
    tpm, fpkm (n = M), gene_tpm, gene_fpkm (n = m) and, with trans_starts, iso_tpm, iso_fpkm; plus 'profile'."""
    cvecs = np.ascontiguousarray(cvecs, np.int32)
    nCV, M1 = cvecs.shape
    M = M1 - 1
    out, gs, m, ts, mt = _ci_outputs(M, gene_starts, trans_starts)
    prof = CiProfile()
    _check(lib().rsem_ci_calculate(device, M, nCV, nSpC, cvecs, np.ascontiguousarray(eel, np.float64),
                                   np.ascontiguousarray(mw, np.float64), float(pseudoC), int(seed), float(confidence), m, gs, mt,
                                   _ptr(ts), out["tpm"], out["fpkm"], out["gene_tpm"], out["gene_fpkm"], _ptr(out.get("iso_tpm")),
                                   _ptr(out.get("iso_fpkm")), C.addressof(prof)))
    out["profile"] = prof
    return out


def ci_calculate_samples(tpm_samples, l_bars, gene_starts, confidence=0.95, trans_starts=None, device=0):
    """Phase II of calcCI.cpp alone (--ci-stream reference): the intervals of the caller's (M, nSamples) float32 TPM samples and
    their l_bars.  Returns what ci_calculate returns."""
    tpm_samples = np.ascontiguousarray(tpm_samples, np.float32)
    M, nS = tpm_samples.shape
    l_bars = np.ascontiguousarray(l_bars, np.float32)
    assert l_bars.shape == (nS,)
    out, gs, m, ts, mt = _ci_outputs(M, gene_starts, trans_starts)
    prof = CiProfile()
    _check(lib().rsem_ci_calculate_samples(device, M, nS, tpm_samples, l_bars, float(confidence), m, gs, mt, _ptr(ts), out["tpm"],
                                           out["fpkm"], out["gene_tpm"], out["gene_fpkm"], _ptr(out.get("iso_tpm")),
                                           _ptr(out.get("iso_fpkm")), C.addressof(prof)))
    out["profile"] = prof
    return out


class Gmap:
    """rsem_gmap: transcript coordinates -> genome coordinates and the per-read collapse of rsem-tbam2gbam.  strand: '+' / '-' per
    transcript (a str, bytes or uint8 array); exon_off: n + 1 offsets into exon_start / exon_end (1-based, inclusive)."""

    def __init__(self, strand, length, out_tid, exon_off, exon_start, exon_end, device=0):
        if isinstance(strand, str):
            strand = strand.encode()
        self.strand = np.frombuffer(strand, np.uint8).copy() if isinstance(strand, (bytes, bytearray)) else np.ascontiguousarray(strand, np.uint8)
        self.length = np.ascontiguousarray(length, np.int32)
        self.out_tid = np.ascontiguousarray(out_tid, np.int32)
        self.exon_off = np.ascontiguousarray(exon_off, np.uint64)
        self.exon_start = np.ascontiguousarray(exon_start, np.int32)
        self.exon_end = np.ascontiguousarray(exon_end, np.int32)
        n = len(self.length)
        assert len(self.strand) == n and len(self.out_tid) == n and len(self.exon_off) == n + 1
        assert len(self.exon_start) == len(self.exon_end) and (n == 0 or len(self.exon_start) >= int(self.exon_off[-1]))
        self.h = C.c_void_p()
        _check(lib().rsem_gmap_create(C.byref(self.h), device, n, _ptr(self.strand), _ptr(self.length), _ptr(self.out_tid), _ptr(self.exon_off),
                                      _ptr(self.exon_start), _ptr(self.exon_end)))

    def convert(self, mates, group_off, tr, pos, l_qseq, flag, w):
        """rsem_gmap_convert.  Returns a dict: per mate tid, pos, flag, n_cigar, bin, has_n; cigar_off (mates + 1) and cigar (the words);
        out_src, out_w (the kept alignments in output order, their folded weights); info."""
        group_off = np.ascontiguousarray(group_off, np.uint64)
        tr, pos, l_qseq = (np.ascontiguousarray(x, np.int32) for x in (tr, pos, l_qseq))
        flag = np.ascontiguousarray(flag, np.uint32)
        w = np.ascontiguousarray(w, np.float32)
        n_aln, n_mates = len(w), len(tr)
        assert n_mates == n_aln * mates or mates not in (1, 2)
        assert len(pos) == n_mates and len(l_qseq) == n_mates and len(flag) == n_mates and len(group_off) >= 1
        ok = (tr >= 0) & (tr < len(self.length))
        exons = (self.exon_off[1:] - self.exon_off[:-1]).astype(np.int64)
        cap = int(np.sum(2 * exons[tr[ok]] + 2)) if n_mates else 0  # the bound include/rsem_hip.h states
        o = {k: np.zeros(n_mates, t) for k, t in (("tid", np.int32), ("pos", np.int32), ("flag", np.uint32), ("n_cigar", np.uint32),
                                                  ("bin", np.uint32), ("has_n", np.uint32))}
        cigar_off = np.zeros(n_mates + 1, np.uint64)
        cigar = np.zeros(max(cap, 1), np.uint32)
        out_src, out_w = np.zeros(max(n_aln, 1), np.uint64), np.zeros(max(n_aln, 1), np.float32)
        info = GmapInfo()
        _check(lib().rsem_gmap_convert(self.h, mates, n_aln, len(group_off) - 1, _ptr(group_off), _ptr(tr), _ptr(pos), _ptr(l_qseq), _ptr(flag), _ptr(w),
                                       _ptr(o["tid"]), _ptr(o["pos"]), _ptr(o["flag"]), _ptr(o["n_cigar"]), _ptr(o["bin"]), _ptr(o["has_n"]),
                                       _ptr(cigar_off), _ptr(cigar), cap, _ptr(out_src), _ptr(out_w), C.addressof(info)))
        o["cigar_off"] = cigar_off
        o["cigar"] = cigar[:int(cigar_off[-1])]
        o["out_src"], o["out_w"] = out_src[:info.n_alignments_out], out_w[:info.n_alignments_out]
        o["info"] = {f: getattr(info, f) for f, _ in GmapInfo._fields_}
        return o

    def close(self):
        if self.h:
            lib().rsem_gmap_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


REFSEQ_RAW, REFSEQ_CHECKED = 0, 1
REFSEQ_RC, REFSEQ_UPPER_N, REFSEQ_N2G, REFSEQ_FILL = 1, 2, 4, 8


class Refseq:
    """rsem_refseq: FASTA bodies -> bases (load) and segments of bases -> an output store (gather) of the reference-preparation
    programs.  store_bytes: the size of the store."""

    def __init__(self, store_bytes, device=0):
        self.store_bytes = int(store_bytes)
        self.h = C.c_void_p()
        _check(lib().rsem_refseq_create(C.byref(self.h), device, self.store_bytes))

    def load(self, mode, raw, body_lo, body_hi, keep=None, first=0):
        """rsem_refseq_load from record `first` on.  Returns (n_taken, n_bases, bad): the arrays have an element per record of the call,
        those of the records taken are filled."""
        self._raw = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, np.uint8)
        lo, hi = np.ascontiguousarray(body_lo, np.uint64), np.ascontiguousarray(body_hi, np.uint64)
        assert len(lo) == len(hi)
        kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        n_bases, bad = np.zeros(max(len(lo), 1), np.uint64), np.full(max(len(lo), 1), -1, np.int64)
        taken = C.c_int64(0)
        _check(lib().rsem_refseq_load(self.h, mode, _ptr(self._raw), len(lo), _ptr(lo), _ptr(hi), _ptr(kp), first, C.byref(taken), _ptr(n_bases), _ptr(bad)))
        return taken.value, n_bases[:len(lo)], bad[:len(lo)]

    def gather(self, src, first_base, length, dst, flags):
        src = np.ascontiguousarray(src, np.int64)
        first_base, length, flags = (np.ascontiguousarray(x, np.uint32) for x in (first_base, length, flags))
        dst = np.ascontiguousarray(dst, np.uint64)
        assert len(src) == len(first_base) == len(length) == len(dst) == len(flags)
        _check(lib().rsem_refseq_gather(self.h, len(src), _ptr(src), _ptr(first_base), _ptr(length), _ptr(dst), _ptr(flags)))

    def run(self, mode, raw, body_lo, body_hi, segments, keep=None):
        """Every record through load, batch after batch, each batch followed by the segments (src, first_base, len, dst, flags) that
        read from it, in the order given; the fills go with the first batch.  Returns (n_bases, bad)."""
        n = len(body_lo)
        seg = np.array(segments, np.int64).reshape(-1, 5)
        first, n_bases, bad = 0, np.zeros(n, np.uint64), np.full(n, -1, np.int64)
        while first < n:
            taken, nb, bd = self.load(mode, raw, body_lo, body_hi, keep, first)
            n_bases[first:first + taken], bad[first:first + taken] = nb[first:first + taken], bd[first:first + taken]
            fill = (seg[:, 4] & REFSEQ_FILL) != 0
            here = (fill & (first == 0)) | (~fill & (seg[:, 0] >= first) & (seg[:, 0] < first + taken))
            g = seg[here]
            if len(g):
                self.gather(g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4])
            first += taken
        return n_bases, bad

    def download(self, offset=0, nbytes=None):
        nbytes = self.store_bytes - offset if nbytes is None else nbytes
        out = np.zeros(max(nbytes, 1), np.uint8)
        _check(lib().rsem_refseq_download(self.h, offset, nbytes, _ptr(out)))
        return out[:nbytes].tobytes()

    def info(self):
        info = RefseqInfo()
        _check(lib().rsem_refseq_get_info(self.h, C.addressof(info)))
        return {f: getattr(info, f) for f, _ in RefseqInfo._fields_}

    def close(self):
        if self.h:
            lib().rsem_refseq_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


(ALNCHECK_OK, ALNCHECK_MIXED, ALNCHECK_ONE_MATE, ALNCHECK_SAME_MATE_NUMBER, ALNCHECK_ONE_MATE_ALIGNED, ALNCHECK_DISCORDANT, ALNCHECK_SAME_STRAND,
 ALNCHECK_PAIR_BOUNDARY, ALNCHECK_CIGAR_SKIP, ALNCHECK_CIGAR_INDEL, ALNCHECK_CIGAR_CLIP, ALNCHECK_BOUNDARY, ALNCHECK_NOT_GROUPED, ALNCHECK_DIFFERENT_LENGTHS) = range(14)


class Alncheck:
    """rsem_alncheck: the checks of rsem-sam-validator as a stream of pushes.  target_len: the header's sequence lengths."""

    def __init__(self, target_len, device=0):
        self.target_len = np.ascontiguousarray(target_len, np.uint32)
        self.h = C.c_void_p()
        _check(lib().rsem_alncheck_create(C.byref(self.h), device, len(self.target_len), _ptr(self.target_len)))

    def push(self, name_off, names, flag, tid, pos, isize, l_qseq, cigar_off, cigar, last=False):
        """rsem_alncheck_push.  Returns the verdict as a dict."""
        name_off, cigar_off = np.ascontiguousarray(name_off, np.uint64), np.ascontiguousarray(cigar_off, np.uint64)
        names = np.frombuffer(names, np.uint8) if isinstance(names, (bytes, bytearray)) else np.ascontiguousarray(names, np.uint8)
        flag, cigar = np.ascontiguousarray(flag, np.uint32), np.ascontiguousarray(cigar, np.uint32)
        tid, pos, isize, l_qseq = (np.ascontiguousarray(x, np.int32) for x in (tid, pos, isize, l_qseq))
        n = len(flag)
        assert len(name_off) == n + 1 and len(cigar_off) == n + 1 and len(tid) == n and len(pos) == n and len(isize) == n and len(l_qseq) == n
        v = AlncheckVerdict()
        _check(lib().rsem_alncheck_push(self.h, n, _ptr(name_off), _ptr(names), _ptr(flag), _ptr(tid), _ptr(pos), _ptr(isize), _ptr(l_qseq), _ptr(cigar_off), _ptr(cigar),
                                        1 if last else 0, C.addressof(v)))
        return {f: getattr(v, f) for f, _ in AlncheckVerdict._fields_}

    def close(self):
        if self.h:
            lib().rsem_alncheck_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def alncheck_unique(name_off, names, flag, device=0):
    """rsem_alncheck_unique: (keep, info) -- per record whether rsem-get-unique writes it."""
    name_off = np.ascontiguousarray(name_off, np.uint64)
    names = np.frombuffer(names, np.uint8) if isinstance(names, (bytes, bytearray)) else np.ascontiguousarray(names, np.uint8)
    flag = np.ascontiguousarray(flag, np.uint32)
    n = len(flag)
    assert len(name_off) == n + 1
    keep = np.zeros(max(n, 1), np.uint8)
    info = AlncheckInfo()
    _check(lib().rsem_alncheck_unique(device, n, _ptr(name_off), _ptr(names), _ptr(flag), _ptr(keep), C.addressof(info)))
    return keep[:n], {f: getattr(info, f) for f, _ in AlncheckInfo._fields_}


PAIRSCAN_OK, PAIRSCAN_MIXED, PAIRSCAN_ODD_FULL, PAIRSCAN_ODD_PARTIAL, PAIRSCAN_NO_PARTNER = range(5)


class Pairscan:
    """rsem_pairscan: the order in which rsem-scan-for-paired-end-reads writes the records of a name-grouped file.  The handle keeps
    its device buffers between calls."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().rsem_pairscan_create(C.byref(self.h), device))

    def reorder(self, name_off, names, flag, tid, pos, mpos, last=False):
        """rsem_pairscan_reorder over whole runs of equal canonical names.  Returns (perm, verdict as a dict): perm[k] is the input
        index of the k-th output record (unspecified where verdict["code"] != 0)."""
        name_off = np.ascontiguousarray(name_off, np.uint64)
        names = np.frombuffer(names, np.uint8) if isinstance(names, (bytes, bytearray)) else np.ascontiguousarray(names, np.uint8)
        flag = np.ascontiguousarray(flag, np.uint32)
        tid, pos, mpos = (np.ascontiguousarray(x, np.int32) for x in (tid, pos, mpos))
        n = len(flag)
        assert len(name_off) == n + 1 and len(tid) == n and len(pos) == n and len(mpos) == n
        perm = np.zeros(max(n, 1), np.uint32)
        v = PairscanVerdict()
        _check(lib().rsem_pairscan_reorder(self.h, n, _ptr(name_off), _ptr(names), _ptr(flag), _ptr(tid), _ptr(pos), _ptr(mpos), 1 if last else 0, _ptr(perm),
                                           C.addressof(v)))
        return perm[:n], {f: getattr(v, f) for f, _ in PairscanVerdict._fields_}

    def close(self):
        if self.h:
            lib().rsem_pairscan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SIM_OK, SIM_ATTEMPT_CAP, SIM_SHORT_INSERT, SIM_PAST_PROFILE, SIM_QUALITY_RANGE = range(5)


def sim_knobs():
    """the RSEM_SIM_* knobs in force (rsem_sim_read_knobs)"""
    k = SimKnobs()
    _check(lib().rsem_sim_read_knobs(C.addressof(k)))
    return {f: getattr(k, f) for f, _ in SimKnobs._fields_}


class Simulate:
    """rsem_sim: reads drawn from a read model after startSimulation.  tables: a dict with type, prob_f, theta_cdf, full_len, tot_len
    (index 0 unused), seqs (a list of M + 1 strings or bytes, [0] unused), g_lb, g_ub, g_cdf and, where the model has them, m_lb, m_ub,
    m_cdf, est_rspd with r_pdf and r_cdf (B + 2 entries), qc_init, qc_trans, pc, npc -- every table a running sum, flat or nested."""

    def __init__(self, tables, device=0):
        t = tables
        f64 = lambda k: None if t.get(k) is None else np.ascontiguousarray(np.asarray(t[k], np.float64).reshape(-1))  # noqa: E731
        self.M = len(t["full_len"]) - 1
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in t["seqs"]]
        off = np.zeros(self.M + 2, np.uint64)
        off[1:] = np.cumsum([0] + [len(s) for s in seqs[1:]])
        keep = {"theta_cdf": f64("theta_cdf"), "full_len": np.ascontiguousarray(t["full_len"], np.int32), "tot_len": np.ascontiguousarray(t["tot_len"], np.int32), "seq_off": off,
                "seq": np.frombuffer(b"".join(seqs[1:]) or b"N", np.uint8), "g_cdf": f64("g_cdf"), "m_cdf": f64("m_cdf"), "r_pdf": f64("r_pdf"), "r_cdf": f64("r_cdf"),
                "qc_init": f64("qc_init"), "qc_trans": f64("qc_trans"), "pc": f64("pc"), "npc": f64("npc")}
        self.type = int(t["type"])
        m = SimModel(type=self.type, M=self.M, has_mld=0 if t.get("m_cdf") is None else 1, est_rspd=1 if t.get("est_rspd") else 0, B=len(keep["r_pdf"]) - 2 if t.get("est_rspd") else 0,
                     pro_len=0 if self.type in (1, 3) else len(keep["pc"]) // 25, g_lb=t["g_lb"], g_ub=t["g_ub"], m_lb=t.get("m_lb", 0), m_ub=t.get("m_ub", 1), prob_f=t["prob_f"])
        for k, a in keep.items():
            setattr(m, k, None if a is None else a.ctypes.data)
        self.h = C.c_void_p()
        _check(lib().rsem_sim_create(C.byref(self.h), C.addressof(m), device))
        ml, plain = C.c_int32(), C.c_int32()
        _check(lib().rsem_sim_info(self.h, C.byref(ml), C.byref(plain)))
        self.max_len, self.plain = ml.value, bool(plain.value)

    def _batch(self, n):
        st = max(self.max_len, 1)
        a = {k: np.zeros(max(n, 1), np.int32) for k in ("sid", "dir", "pos", "insert_l", "len1", "len2")}
        a["attempts"] = np.zeros(max(n, 1), np.uint32)
        for k in ("seq1", "qual1", "seq2", "qual2"):
            a[k] = np.zeros((max(n, 1), st), np.uint8)
        b = SimBatch(capacity=n, stride=st)
        for k, v in a.items():
            setattr(b, k, v.ctypes.data)
        return a, b

    def _result(self, a, b):
        out = {f: getattr(b, f) for f, _ in SimBatch._fields_ if f not in a}
        n = b.n_reads
        out.update({k: v[:n] for k, v in a.items()})
        return out

    def counter_batch(self, seed, first_read, n_reads):
        """rsem_sim_counter_batch -> a dict of the batch's arrays (cut to n_reads) and scalars"""
        a, b = self._batch(n_reads)
        _check(lib().rsem_sim_counter_batch(self.h, seed, first_read, n_reads, C.addressof(b)))
        return self._result(a, b)

    def reference_begin(self, seed):
        _check(lib().rsem_sim_reference_begin(self.h, seed))

    def reference_batch(self, max_reads):
        a, b = self._batch(max_reads)
        _check(lib().rsem_sim_reference_batch(self.h, max_reads, C.addressof(b)))
        return self._result(a, b)

    def totals(self):
        counts, resim = np.zeros(self.M + 1, np.uint64), C.c_uint64()
        _check(lib().rsem_sim_totals(self.h, counts, C.byref(resim)))
        return counts, resim.value

    def close(self):
        if self.h:
            lib().rsem_sim_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
