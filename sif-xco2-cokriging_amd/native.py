"""ctypes binding of libcokrige_hip.so (C ABI: include/cokrige.h).

The library is built in-tree by ``build_native.py`` (hipcc, gfx950).  Loading fails
loudly when it is missing -- there is deliberately no numpy fallback.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# CK_LIB_PATH: load another build of the library (kernel experiments) instead of overwriting the product one
LIB_PATH = os.environ.get("CK_LIB_PATH") or os.path.join(HERE, "libcokrige_hip.so")

METRIC_HAVERSINE = 0
METRIC_EUCLID = 1
PANEL_SLACK_BYTES = 64 * 512 * 8   # include/cokrige.h: CK_PANEL_SLACK_BYTES
APPLY_SIGMA = 1
APPLY_AUX = 2

_dp = POINTER(c_double)
_lib = None

# name -> argtypes (every function returns int except ck_last_error)
_PROTOS = {
    "ck_version": [],
    "ck_device_count": [POINTER(c_int)],
    "ck_create": [c_int, POINTER(c_void_p)],
    "ck_create_partitioned": [POINTER(c_int), c_int, c_int, POINTER(c_void_p)],
    "ck_destroy": [c_void_p],
    "ck_set_stream": [c_void_p, c_void_p, c_int],
    "ck_set_arena": [c_void_p, c_void_p, c_int64],
    "ck_synchronize": [c_void_p],
    "ck_estimate_bytes": [c_void_p, c_int64, POINTER(c_int64)],
    "ck_set_model": [c_void_p, c_int, _dp, _dp, _dp, _dp, c_double],
    "ck_set_metric": [c_void_p, c_int],
    "ck_set_partition": [c_void_p, c_int, c_int],
    "ck_set_data": [c_void_p, c_int, _dp, _dp, c_int64],
    "ck_distance_dense": [c_void_p, _dp, c_int64, _dp, c_int64, _dp],
    "ck_cov_dense": [c_void_p, c_int, c_int, _dp, c_int64, _dp, c_int64, c_int, _dp],
    "ck_cov_lags": [c_void_p, c_int, c_int, _dp, c_int64, c_int, _dp],
    "ck_model_variogram": [c_void_p, POINTER(c_int32), POINTER(c_int32), _dp, c_int64, c_int, _dp],
    "ck_assemble_joint": [c_void_p],
    "ck_factor": [c_void_p, POINTER(c_int64)],
    "ck_predict": [c_void_p, c_int, _dp, c_int64, _dp, _dp],
    "ck_factor_predict": [c_void_p, c_int, _dp, c_int64, _dp, _dp, POINTER(c_int64)],
    "ck_verify_model": [c_void_p, POINTER(c_int64)],
    "ck_predict_blocks": [c_void_p, c_int, _dp, c_int64, POINTER(c_int32), _dp, c_int32, _dp, _dp, _dp],
    "ck_loocv": [c_void_p, c_int, _dp, _dp],
    "ck_cv_folds": [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), c_int32, _dp, _dp, _dp, POINTER(c_int64)],
    "ck_loglik": [c_void_p, c_int, _dp, _dp, POINTER(c_int64)],
    "ck_set_trend": [c_void_p, c_int, _dp, c_int64, c_int],
    "ck_set_noise": [c_void_p, c_int, _dp, c_int64, c_double],
    "ck_loglik_noise_grad": [c_void_p, _dp],
    "ck_predict_universal": [c_void_p, c_int, _dp, c_int64, _dp, _dp, _dp, _dp, _dp],
    "ck_loglik_reml": [c_void_p, c_int, _dp, _dp, POINTER(c_int64)],
    "ck_loglik_fisher": [c_void_p, c_int, POINTER(c_int32), _dp, POINTER(c_int64)],
    "ck_sample": [c_void_p, _dp, _dp, c_int64],
    "ck_conditional_draws": [c_void_p, c_int, _dp, c_int64, c_int64, c_uint64, _dp, c_double, c_double, _dp, _dp, _dp,
                             POINTER(c_uint8), POINTER(c_int64)],
    "ck_predict_pair": [c_void_p, _dp, c_int64, _dp, c_int64, _dp, _dp, _dp, _dp, POINTER(c_int64), c_int64, _dp],
    "ck_conditional_draws_pair": [c_void_p, _dp, c_int64, _dp, c_int64, c_int64, c_uint64, _dp, c_double, c_double, _dp, _dp,
                                  _dp, POINTER(c_uint8), POINTER(c_int64)],
    "ck_num_panels": [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int64)],
    "ck_panel_owner": [c_void_p, c_int, POINTER(c_int)],
    "ck_aux_begin": [c_void_p, c_int, _dp, c_int64],
    "ck_panel_factor": [c_void_p, c_int],
    "ck_panel_buffer": [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int64)],
    "ck_panel_apply": [c_void_p, c_int, c_int],
    "ck_panel_apply_sigma": [c_void_p, c_int, c_int, c_int],
    "ck_panel_apply_group": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int],
    "ck_panel_aux_solve": [c_void_p, c_int],
    "ck_aux_finish": [c_void_p, _dp, _dp],
    "ck_factor_info": [c_void_p, POINTER(c_int64)],
    "ck_predict_local": [c_void_p, c_int, _dp, c_int64, c_double, c_int, _dp, _dp, POINTER(c_int64), POINTER(c_int64),
                         POINTER(c_int64)],
    "ck_local_reserve": [c_void_p, c_int64],
    "ck_set_local_neighbours": [c_void_p, c_int64, c_int64],
    "ck_debug_local_neighbours": [c_void_p, c_int, _dp, c_int64, c_double, c_int, POINTER(c_int32), _dp],
    "ck_cv_local_folds": [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), c_int32, _dp, _dp, c_double, _dp, _dp, _dp, _dp, _dp,
                          POINTER(c_int64)],
    "ck_debug_local_cv_neighbours": [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), c_int32, _dp, c_double, POINTER(c_int32),
                                     _dp],
    "ck_loglik_vecchia": [c_void_p, POINTER(c_int64), c_double, _dp, _dp, _dp, POINTER(c_int32), POINTER(c_int64),
                          POINTER(c_int64)],
    "ck_loglik_vecchia_grad": [c_void_p, POINTER(c_int64), c_double, POINTER(c_int32), _dp, _dp, _dp, POINTER(c_int64),
                               POINTER(c_int64)],
    "ck_loglik_vecchia_fisher": [c_void_p, POINTER(c_int64), c_double, POINTER(c_int32), _dp, POINTER(c_int64), POINTER(c_int64)],
    "ck_loglik_vecchia_trend": [c_void_p, POINTER(c_int64), c_double, c_int, _dp, _dp, _dp, _dp, _dp, POINTER(c_int32),
                                POINTER(c_int64), POINTER(c_int64)],
    "ck_loglik_vecchia_trend_grad": [c_void_p, POINTER(c_int64), c_double, POINTER(c_int32), _dp, _dp, _dp, _dp, _dp,
                                     POINTER(c_int64), POINTER(c_int64)],
    "ck_debug_vecchia_trend": [c_void_p, POINTER(c_int64), c_double, _dp, _dp, _dp],
    "ck_predict_local_universal": [c_void_p, c_int, _dp, c_int64, _dp, c_double, c_int, _dp, _dp, _dp, POINTER(c_int64),
                                   POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)],
    "ck_predict_local_pair": [c_void_p, _dp, c_int64, c_double, _dp, _dp, _dp, _dp, _dp, POINTER(c_int64), POINTER(c_int64),
                              POINTER(c_int64)],
    "ck_predict_local_blocks": [c_void_p, c_int, _dp, c_int32, _dp, c_int64, POINTER(c_int32), _dp, _dp, c_double, _dp, _dp, _dp,
                                POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)],
    "ck_simulate_local": [c_void_p, c_int, _dp, c_int64, POINTER(c_int64), c_double, c_int64, c_uint64, _dp, _dp, _dp, _dp,
                          POINTER(c_int32), POINTER(c_int64), POINTER(c_int64)],
    "ck_debug_simulate_local_weights": [c_void_p, c_int, _dp, c_int64, POINTER(c_int64), c_double, POINTER(c_int64), _dp],
    "ck_simulate_local_pair": [c_void_p, _dp, c_int64, _dp, c_int64, POINTER(c_int64), c_double, c_int64, c_uint64, _dp, _dp, _dp,
                               _dp, POINTER(c_int32), POINTER(c_int64), POINTER(c_int64)],
    "ck_debug_simulate_local_pair_weights": [c_void_p, _dp, c_int64, _dp, c_int64, POINTER(c_int64), c_double, POINTER(c_int64),
                                             _dp],
    "ck_vario_begin": [c_void_p, _dp, _dp, c_int64, _dp, _dp, c_int64, c_int],
    "ck_vario_extent": [c_void_p, c_double, _dp, _dp, POINTER(c_int64)],
    "ck_vario_bin": [c_void_p, c_double, _dp, c_int, c_int, _dp, POINTER(c_int64)],
    "ck_vario_end": [c_void_p],
    "ck_vario_stats": [c_void_p, POINTER(c_int64), c_int],
    "ck_ref_distance": [c_int, _dp, _dp, c_int64, _dp],
    "ck_hilbert_order": [_dp, c_int64, POINTER(c_int64)],
    "ck_debug_matern_grad": [c_void_p, c_int, _dp, c_int64, _dp],
    "ck_debug_get_lower": [c_void_p, _dp, c_int64],
    "ck_debug_site_order": [c_void_p, c_int, POINTER(c_int64), c_int64],
    "ck_debug_get_entries": [c_void_p, POINTER(c_int64), POINTER(c_int64), c_int64, _dp],
    "ck_debug_mfma_probe": [c_void_p, POINTER(c_int32)],
    "ck_debug_potrf_profile": [c_void_p, c_int, _dp],
    "ck_debug_coop_profile": [c_void_p, c_int64, _dp],
    "ck_debug_mfma_peak": [c_void_p, c_int, c_int, _dp],
    "ck_debug_gemm_clock": [c_void_p, _dp],
    "ck_debug_stream_overlap": [c_void_p, c_int, c_int64, c_int, _dp],
    "ck_debug_tile_map": [c_int64, c_int, c_int, c_int, POINTER(c_int32), c_int64],
    "ck_debug_tall_map": [c_int64, c_int, c_int, c_int, POINTER(c_int32), c_int64],
    "ck_debug_run_map": [POINTER(c_int32), c_int, POINTER(c_int32), c_int64],
    "ck_debug_gemm_stamps": [c_void_p, POINTER(c_uint64), c_int64, POINTER(c_int64)],
    "ck_debug_cu_probe": [c_void_p, POINTER(c_uint32), c_int, POINTER(c_uint32)],
    "ck_set_option": [c_void_p, c_char_p, c_int64],
    "ck_timings": [c_void_p, _dp, c_int],
    "ck_table_fallbacks": [c_void_p, c_int, POINTER(c_int64)],
    "ck_table_info": [c_void_p, c_int, POINTER(c_int), POINTER(c_int), _dp, _dp, _dp],
    "ck_dev_gemm_nt": [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                       c_int],
}


class NativeError(RuntimeError):
    pass


def exported_names():
    """Every symbol include/cokrige.h declares (used by the symbol-export test)."""
    return ["ck_last_error"] + list(_PROTOS)


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (SONAME libamdhip64.so.7, same as /opt/rocm's) but load it by the unversioned file name,
    so whichever of {torch, this library} comes second would otherwise map a SECOND runtime,
    which then sees no GPU.  When torch is installed, map its copy first (by path, global):
    our NEEDED libamdhip64.so.7 and torch's later dlopen both resolve to it."""
    import importlib.util
    import sys
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


_RET_INT64 = {"ck_debug_tile_map", "ck_debug_tall_map", "ck_debug_run_map"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `python sif-xco2-cokriging_amd/build_native.py` "
                "(hipcc, gfx950).  There is no CPU fallback.")
        _preload_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        L.ck_last_error.restype = c_char_p
        L.ck_last_error.argtypes = []
        for name, args in _PROTOS.items():
            fn = getattr(L, name)
            fn.restype = c_int64 if name in _RET_INT64 else c_int
            fn.argtypes = args
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise NativeError(lib().ck_last_error().decode("utf-8", "replace"))


def _f64(a, shape2=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape2 is not None:
        a = a.reshape(-1, shape2)
    return a


def _p(a):
    return a.ctypes.data_as(_dp)


def ref_distance(metric: int, A, B):
    """The reference's distance arithmetic for n coordinate pairs on the host (libm), bit for bit
    src/fields.py:332-342 -- what decides variogram ties (include/cokrige.h: ck_ref_distance)."""
    A, B = _f64(A, 2), _f64(B, 2)
    if A.shape != B.shape:
        raise ValueError("A and B must have the same shape")
    out = np.empty(A.shape[0])
    _chk(lib().ck_ref_distance(int(metric), _p(A), _p(B), A.shape[0], _p(out)))
    return out


def tile_map(nvalid: int, J0: int, Jstep: int, nJ: int):
    """(block column, tile row, tile column) of every workgroup of one Cholesky trailing update, in launch order
    (include/cokrige.h: ck_debug_tile_map; host only)."""
    n = lib().ck_debug_tile_map(int(nvalid), int(J0), int(Jstep), int(nJ), None, 0)
    if n < 0:
        _chk(-1)
    out = np.zeros((n, 3), dtype=np.int32)
    if n:
        lib().ck_debug_tile_map(int(nvalid), int(J0), int(Jstep), int(nJ), out.ctypes.data_as(POINTER(c_int32)), n)
    return out


def tall_map(nvalid: int, J0: int, nJ: int, aux_tile_rows: int):
    """(block column, tile row, tile column, is right-hand-side tile) of every workgroup of one update of the tall matrix
    [Sigma; c0^T; z^T] (include/cokrige.h: ck_debug_tall_map; host only)."""
    n = lib().ck_debug_tall_map(int(nvalid), int(J0), int(nJ), int(aux_tile_rows), None, 0)
    if n < 0:
        _chk(-1)
    out = np.zeros((n, 4), dtype=np.int32)
    if n:
        lib().ck_debug_tall_map(int(nvalid), int(J0), int(nJ), int(aux_tile_rows), out.ctypes.data_as(POINTER(c_int32)), n)
    return out


def run_map(counts):
    """(system, unit) of every workgroup of a batched launch over systems with `counts` units each, -1 for padding
    workgroups (include/cokrige.h: ck_debug_run_map; host only)."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    cp = c.ctypes.data_as(POINTER(c_int32))
    n = lib().ck_debug_run_map(cp, c.size, None, 0)
    if n < 0:
        _chk(-1)
    out = np.zeros((n, 2), dtype=np.int32)
    if n:
        lib().ck_debug_run_map(cp, c.size, out.ctypes.data_as(POINTER(c_int32)), n)
    return out


def hilbert_order(coords):
    """Indices of the sites in the order the library lays them out on the device (include/cokrige.h: ck_hilbert_order;
    host only)."""
    c = _f64(coords, 2)
    perm = np.empty(c.shape[0], dtype=np.int64)
    _chk(lib().ck_hilbert_order(_p(c), c.shape[0], perm.ctypes.data_as(POINTER(c_int64))))
    return perm


def device_count() -> int:
    n = c_int(0)
    _chk(lib().ck_device_count(byref(n)))
    return n.value


class Handle:
    """One GPU, one HIP stream, one cokriging problem (see include/cokrige.h)."""

    def __init__(self, device: int = 0, devices=None, rank: int = 0):
        """device: one GPU, one problem.  devices + rank: this process's handle of a multi-GPU run (one process per
        entry of `devices`), already partitioned (rank, len(devices)) -- include/cokrige.h: ck_create_partitioned."""
        self._h = c_void_p()
        self._keep = []
        self._trend_p, self._n_data = {}, {}
        if devices is None:
            _chk(lib().ck_create(int(device), byref(self._h)))
        else:
            ids = (c_int * len(devices))(*[int(d) for d in devices])
            _chk(lib().ck_create_partitioned(ids, len(devices), int(rank), byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().ck_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ------------------------------------------------------------------
    def set_stream(self, stream_ptr, external=True):
        """Launch on the caller's HIP stream (0 = the legacy default stream torch uses);
        ``external=False`` restores the handle's own stream."""
        _chk(lib().ck_set_stream(self._h, c_void_p(stream_ptr or 0), int(bool(external))))

    def set_arena(self, dev_ptr: int, nbytes: int, keepalive=None):
        self._keep.append(keepalive)
        _chk(lib().ck_set_arena(self._h, c_void_p(dev_ptr), int(nbytes)))

    def estimate_bytes(self, m: int) -> int:
        out = c_int64(0)
        _chk(lib().ck_estimate_bytes(self._h, int(m), byref(out)))
        return out.value

    def synchronize(self):
        _chk(lib().ck_synchronize(self._h))

    def set_option(self, name: str, value: int):
        _chk(lib().ck_set_option(self._h, name.encode(), int(value)))

    def set_model(self, n_procs, sigma, nu, len_scale, nugget, rho12=0.0):
        s, v, l, g = (_f64(x).ravel() for x in (sigma, nu, len_scale, nugget))
        if n_procs == 2 and (s.size != 2 or v.size != 3 or l.size != 3 or g.size != 2):
            raise ValueError("bivariate model needs sigma[2], nu[3], len_scale[3], nugget[2]")
        _chk(lib().ck_set_model(self._h, int(n_procs), _p(s), _p(v), _p(l), _p(g), float(rho12)))
        self._n_procs = int(n_procs)

    def set_metric(self, metric: int):
        _chk(lib().ck_set_metric(self._h, int(metric)))

    def set_partition(self, rank: int, world: int):
        _chk(lib().ck_set_partition(self._h, int(rank), int(world)))

    def set_data(self, k: int, coords, values):
        c = _f64(coords, 2)
        v = _f64(values).ravel()
        if c.shape[0] != v.size:
            raise ValueError("coords and values disagree in length")
        _chk(lib().ck_set_data(self._h, int(k), _p(c), _p(v), c.shape[0]))
        self._n_data[int(k)] = c.shape[0]
        self._trend_p[int(k)] = 0   # ck_set_data clears the trend of process k

    # -- element-wise surface -------------------------------------------------------------
    def distance_dense(self, A, B):
        A, B = _f64(A, 2), _f64(B, 2)
        out = np.empty((A.shape[0], B.shape[0]))
        _chk(lib().ck_distance_dense(self._h, _p(A), A.shape[0], _p(B), B.shape[0], _p(out)))
        return out

    def cov_dense(self, i, j, A, B, use_nugget=True):
        A, B = _f64(A, 2), _f64(B, 2)
        out = np.empty((A.shape[0], B.shape[0]))
        _chk(lib().ck_cov_dense(self._h, int(i), int(j), _p(A), A.shape[0], _p(B), B.shape[0], int(bool(use_nugget)),
                                _p(out)))
        return out

    def cov_lags(self, i, j, h, use_nugget=True):
        h = _f64(h)
        out = np.empty(h.shape)
        _chk(lib().ck_cov_lags(self._h, int(i), int(j), _p(h.ravel()), h.size, int(bool(use_nugget)), _p(out)))
        return out

    def model_variogram(self, i, j, h, kind="semivariogram"):
        """Row-wise model (cross-)variogram values (src/model.py:209-237) in one launch."""
        h = _f64(h).ravel()
        ii = np.ascontiguousarray(np.broadcast_to(np.asarray(i, dtype=np.int32), h.shape))
        jj = np.ascontiguousarray(np.broadcast_to(np.asarray(j, dtype=np.int32), h.shape))
        out = np.empty(h.shape)
        _chk(lib().ck_model_variogram(self._h, ii.ctypes.data_as(POINTER(c_int32)), jj.ctypes.data_as(POINTER(c_int32)),
                                      _p(h), h.size, 1 if kind == "covariogram" else 0, _p(out)))
        return out

    # -- joint path -------------------------------------------------------------------------
    def assemble_joint(self):
        _chk(lib().ck_assemble_joint(self._h))

    def factor(self) -> int:
        info = c_int64(0)
        _chk(lib().ck_factor(self._h, byref(info)))
        return info.value

    def predict(self, i, pcoords):
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        pred, err = np.empty(m), np.empty(m)
        _chk(lib().ck_predict(self._h, int(i), _p(pc), m, _p(pred), _p(err)))
        return pred, err

    def factor_predict(self, i, pcoords):
        """factor() + predict() with the two sweeps overlapped (include/cokrige.h: ck_factor_predict).  Returns
        (info, pred, err); info != 0: Sigma is not positive definite, pred / err are meaningless."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        pred, err = np.empty(m), np.empty(m)
        info = c_int64(0)
        _chk(lib().ck_factor_predict(self._h, int(i), _p(pc), m, _p(pred), _p(err), byref(info)))
        return info.value, pred, err

    def verify_model(self) -> int:
        """0 if the joint covariance of data and the last predict()'s sites is positive definite, else the index
        of the failing minor (src/joint_prediction.py:260-274; include/cokrige.h: ck_verify_model)."""
        info = c_int64(0)
        _chk(lib().ck_verify_model(self._h, byref(info)))
        return info.value

    def predict_blocks(self, i, pcoords, block, weight, r, want_cov=False):
        """Weighted regional means of process i on the resident factor (include/cokrige.h: ck_predict_blocks):
        block[a] in [0, r) names the block of site a, weight[a] its weight.  Returns (pred, err, cov | None), r values
        each and with ``want_cov`` the r x r covariance A S A^T of the block predictions."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        b = np.ascontiguousarray(block, dtype=np.int32).ravel()
        w = _f64(weight).ravel()
        if b.size != m or w.size != m:
            raise ValueError("pcoords, block and weight disagree in length")
        r = int(r)
        pred, err = np.empty(max(r, 0)), np.empty(max(r, 0))
        cov = np.empty((r, r)) if want_cov and r > 0 else None
        _chk(lib().ck_predict_blocks(self._h, int(i), _p(pc), m, b.ctypes.data_as(POINTER(c_int32)), _p(w), r, _p(pred),
                                     _p(err), _p(cov) if cov is not None else None))
        return pred, err, cov

    def loglik(self, want_grad=False):
        """Gaussian log-likelihood of the loaded data under the model (include/cokrige.h: ck_loglik) on an assembled handle.
        Returns (info, (l, log|Sigma|, z^T Sigma^-1 z), gradient | None); info != 0: Sigma is not positive definite (the
        1-based leading minor) and the values are NaN.  The gradient is in MaternParams' flat order (11 or 4 values)."""
        out3 = np.empty(3)
        grad = np.empty(11) if want_grad else None
        info = c_int64(0)
        _chk(lib().ck_loglik(self._h, int(bool(want_grad)), _p(out3), _p(grad) if grad is not None else None, byref(info)))
        if grad is not None and getattr(self, "_n_procs", 2) == 1:
            grad = grad[:4].copy()
        return info.value, tuple(out3.tolist()), grad

    def set_trend(self, k, F):
        """Regressors of process k at its data sites, (n_k, p_k) in the order of set_data (include/cokrige.h: ck_set_trend);
        None or p_k = 0 clears the trend of process k."""
        if F is None:
            n = int(getattr(self, "_n_data", {}).get(int(k), 0))
            _chk(lib().ck_set_trend(self._h, int(k), None, n, 0))
            self._trend_p[int(k)] = 0
            return
        F = _f64(F)
        if F.ndim != 2:
            raise ValueError("the regressors must be a 2-D array (n_k, p_k)")
        _chk(lib().ck_set_trend(self._h, int(k), _p(F) if F.size else None, F.shape[0], F.shape[1]))
        self._trend_p[int(k)] = F.shape[1]

    def set_noise(self, k, var, scale=1.0):
        """Measurement-error variances of the data of process k, (n_k,) in the order of set_data, and their scale: Sigma gets
        scale * var on its true diagonal (include/cokrige.h: ck_set_noise).  None clears them.  Sigma must be assembled
        again afterwards."""
        if var is None:
            _chk(lib().ck_set_noise(self._h, int(k), None, 0, 1.0))
            return
        v = _f64(var).ravel()
        _chk(lib().ck_set_noise(self._h, int(k), _p(v) if v.size else None, v.size, float(scale)))

    def loglik_noise_grad(self):
        """(dl/ds_0, dl/ds_1): the derivatives of the last loglik() / loglik_reml() with a gradient in the noise scales
        (include/cokrige.h: ck_loglik_noise_grad); 0 for a process without noise."""
        out = np.empty(2)
        _chk(lib().ck_loglik_noise_grad(self._h, _p(out)))
        return out

    def predict_universal(self, i, pcoords, f0=None):
        """Universal cokriging of process i on the resident factor (include/cokrige.h: ck_predict_universal).  f0: (m, p_i)
        regressors of process i at pcoords.  Returns (pred, err, beta, beta_cov) with beta (p,) and beta_cov (p, p) over the
        trend columns of both processes; without a trend (p = 0) the predict() result and empty beta / beta_cov."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        p = sum(self._trend_p.values())
        pi = self._trend_p.get(int(i), 0)
        F0 = None
        if pi > 0:
            F0 = _f64(np.zeros((m, 0)) if f0 is None else f0)
            if F0.shape != (m, pi):
                raise ValueError(f"f0 has shape {F0.shape}, expected {(m, pi)}")
        pred, err = np.empty(m), np.empty(m)
        beta, cov = np.empty(p), np.empty((p, p))
        _chk(lib().ck_predict_universal(self._h, int(i), _p(pc), m, _p(F0) if F0 is not None else None, _p(pred), _p(err),
                                        _p(beta) if p else None, _p(cov) if p else None))
        return pred, err, beta, cov

    def universal_timings(self):
        """ck_timings [40 ..] of the last predict_universal() call, in milliseconds."""
        out = np.zeros(46)
        _chk(lib().ck_timings(self._h, _p(out), 46))
        keys = ["k2_ms", "sweep_ms", "reduce_ms", "gls_ms", "finish_ms", "total_ms"]
        return dict(zip(keys, out[40:46].tolist()))

    def loglik_reml(self, want_grad=False):
        """Restricted log-likelihood for the trend of set_trend (include/cokrige.h: ck_loglik_reml) on an assembled handle.
        Returns (info, (l_R, log|Sigma|, log|X^T Sigma^-1 X|, z^T P z), gradient | None), as loglik()."""
        out4 = np.empty(4)
        grad = np.empty(11) if want_grad else None
        info = c_int64(0)
        _chk(lib().ck_loglik_reml(self._h, int(bool(want_grad)), _p(out4), _p(grad) if grad is not None else None,
                                  byref(info)))
        if grad is not None and getattr(self, "_n_procs", 2) == 1:
            grad = grad[:4].copy()
        return info.value, tuple(out4.tolist()), grad

    def fisher(self, reml=False, free=None):
        """Expected (Fisher) information of the likelihood at the model's parameters (include/cokrige.h: ck_loglik_fisher) on
        an assembled handle.  ``free``: 13 flags over the slots (11 model parameters in the flat order -- one process: the
        first 4 -- then the noise scales s_0, s_1), None = all.  Returns (info, I) with I the 13 x 13 array: rows and columns of
        slots that are not live are 0; info != 0: Sigma is not positive definite and I is NaN."""
        out = np.empty((13, 13))
        info = c_int64(0)
        fr = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free).astype(bool), dtype=np.int32)
            if fr.shape != (13,):
                raise ValueError("free: 13 flags, one per slot")
        _chk(lib().ck_loglik_fisher(self._h, int(bool(reml)), fr.ctypes.data_as(POINTER(c_int32)) if fr is not None else None,
                                    _p(out), byref(info)))
        return info.value, out

    def fisher_timings(self):
        """ck_timings [64 ..] of the last fisher() call: milliseconds, the flop of the products and the number of groups."""
        out = np.zeros(70)
        _chk(lib().ck_timings(self._h, _p(out), 70))
        keys = ["assemble_ms", "product_ms", "contract_ms", "total_ms", "flop", "groups"]
        return dict(zip(keys, out[64:70].tolist()))

    def loglik_timings(self):
        """ck_timings [24 ..] of the last loglik() call, in milliseconds."""
        out = np.zeros(30)
        _chk(lib().ck_timings(self._h, _p(out), 30))
        keys = ["assemble_ms", "factor_ms", "sweep_ms", "syrk_ms", "contract_ms", "total_ms"]
        return dict(zip(keys, out[24:30].tolist()))

    def conditional_draws(self, i, pcoords, n_draws, seed=0, noise=None, tol=1e-10, jitter=0.0):
        """Draws from the posterior of process i at pcoords on the resident factor (include/cokrige.h: ck_conditional_draws).
        Returns (draws (n_draws, m), pred, pred_err, deflated (bool, m), info); info != 0: S could not be factored at the
        caller's site info - 1 and ``draws`` holds zeros.  ``noise``: (n_draws, m) normals in the caller's order, else the
        device's Philox stream keyed on ``seed``."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        n_draws = int(n_draws)
        e = None
        if noise is not None:
            e = _f64(noise)
            if e.shape != (n_draws, m):
                raise ValueError(f"noise has shape {e.shape}, expected {(n_draws, m)}")
        draws = np.zeros((max(n_draws, 0), m))
        pred, err = np.empty(m), np.empty(m)
        defl = np.zeros(m, dtype=np.uint8)
        info = c_int64(0)
        _chk(lib().ck_conditional_draws(self._h, int(i), _p(pc), m, n_draws, c_uint64(int(seed) & (2 ** 64 - 1)),
                                        _p(e) if e is not None else None, float(tol), float(jitter), _p(draws), _p(pred),
                                        _p(err), defl.ctypes.data_as(POINTER(c_uint8)), byref(info)))
        return draws, pred, err, defl.astype(bool), info.value

    def draws_timings(self):
        """ck_timings [30 ..] of the last conditional_draws() call (milliseconds; the last two are counts)."""
        out = np.zeros(40)
        _chk(lib().ck_timings(self._h, _p(out), 40))
        keys = ["predict_ms", "cpp_ms", "vtv_ms", "deflate_ms", "factor_ms", "noise_ms", "product_ms", "total_ms",
                "n_deflated", "n_chunks"]
        return dict(zip(keys, out[30:40].tolist()))

    def predict_pair(self, pcoords0, pcoords1, pairs=None):
        """Both processes from one forward sweep on the resident factor (include/cokrige.h: ck_predict_pair).  ``pairs``:
        (q, 2) integers (a, b) -- a indexes pcoords0, b indexes pcoords1.  Returns (pred0, err0, pred1, err1, pair_cov | None);
        pair_cov[t] is the posterior covariance between process 0 at site a_t and process 1 at site b_t."""
        pc0, pc1 = _f64(pcoords0, 2), _f64(pcoords1, 2)
        m0, m1 = pc0.shape[0], pc1.shape[0]
        pred0, err0, pred1, err1 = np.empty(m0), np.empty(m0), np.empty(m1), np.empty(m1)
        pr = cov = None
        q = 0
        if pairs is not None:
            pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
            q = pr.shape[0]
            cov = np.empty(q)
        _chk(lib().ck_predict_pair(self._h, _p(pc0), m0, _p(pc1), m1, _p(pred0), _p(err0), _p(pred1), _p(err1),
                                   pr.ctypes.data_as(POINTER(c_int64)) if pr is not None else None, q,
                                   _p(cov) if cov is not None else None))
        return pred0, err0, pred1, err1, cov

    def conditional_draws_pair(self, pcoords0, pcoords1, n_draws, seed=0, noise=None, tol=1e-10, jitter=0.0):
        """Joint draws of both processes (include/cokrige.h: ck_conditional_draws_pair).  Everything is stacked: columns
        [0, m0) are process 0 at pcoords0, [m0, m0 + m1) process 1 at pcoords1.  Returns (draws (n_draws, m0 + m1), pred,
        pred_err, deflated (bool), info); info != 0: S could not be factored at the stacked site info - 1."""
        pc0, pc1 = _f64(pcoords0, 2), _f64(pcoords1, 2)
        m0, m1 = pc0.shape[0], pc1.shape[0]
        m = m0 + m1
        n_draws = int(n_draws)
        e = None
        if noise is not None:
            e = _f64(noise)
            if e.shape != (n_draws, m):
                raise ValueError(f"noise has shape {e.shape}, expected {(n_draws, m)}")
        draws = np.zeros((max(n_draws, 0), m))
        pred, err = np.empty(m), np.empty(m)
        defl = np.zeros(m, dtype=np.uint8)
        info = c_int64(0)
        _chk(lib().ck_conditional_draws_pair(self._h, _p(pc0), m0, _p(pc1), m1, n_draws, c_uint64(int(seed) & (2 ** 64 - 1)),
                                             _p(e) if e is not None else None, float(tol), float(jitter), _p(draws),
                                             _p(pred), _p(err), defl.ctypes.data_as(POINTER(c_uint8)), byref(info)))
        return draws, pred, err, defl.astype(bool), info.value

    def pair_timings(self):
        """ck_timings [124 ..] of the last conditional_draws_pair() and [134 ..] of the last predict_pair() stages."""
        out = np.zeros(138)
        _chk(lib().ck_timings(self._h, _p(out), 138))
        keys = ["predict_ms", "cpp_ms", "vtv_ms", "deflate_ms", "factor_ms", "noise_ms", "product_ms", "total_ms",
                "n_deflated", "n_chunks", "pair_assemble_ms", "pair_sweep_ms", "pair_reduce_ms", "pair_total_ms"]
        return dict(zip(keys, out[124:138].tolist()))

    def loocv(self, i, n_i):
        pred, err = np.empty(n_i), np.empty(n_i)
        _chk(lib().ck_loocv(self._h, int(i), _p(pred), _p(err)))
        return pred, err

    def cv_folds(self, i, folds_i, folds_other=None, n_folds=None, want_stats=False):
        """Leave-group-out cross-validation of process ``i`` from the resident factor (include/cokrige.h: ck_cv_folds).
        ``folds_i`` / ``folds_other``: int labels in [-1, n_folds) of the data of process i / of the other process (the caller's
        order of set_data; -1 = never withheld; ``folds_other=None``: nothing of the other process is withheld).
        Returns (info, pred, pred_err[, fold_stats (n_folds x 3)])."""
        fi = np.ascontiguousarray(folds_i, dtype=np.int32).ravel()
        fo = None if folds_other is None else np.ascontiguousarray(folds_other, dtype=np.int32).ravel()
        if n_folds is None:
            n_folds = int(max(fi.max(initial=-1), -1 if fo is None else fo.max(initial=-1))) + 1
        n_folds = int(n_folds)
        pred, err = np.empty(fi.size), np.empty(fi.size)
        stats = np.empty((max(n_folds, 0), 3)) if want_stats else None
        info = c_int64(0)
        ip = POINTER(c_int32)
        pi = fi.ctypes.data_as(ip)
        po = None if fo is None else fo.ctypes.data_as(ip)
        f0, f1 = (pi, po) if int(i) == 0 else (po, pi)
        _chk(lib().ck_cv_folds(self._h, int(i), f0, f1, n_folds, _p(pred), _p(err), _p(stats) if want_stats else None, byref(info)))
        return (info.value, pred, err, stats) if want_stats else (info.value, pred, err)

    def cv_folds_timings(self):
        """ck_timings [56 ..] of the last cv_folds() call (milliseconds)."""
        out = np.zeros(60)
        _chk(lib().ck_timings(self._h, _p(out), 60))
        return dict(zip(["sweep_ms", "gram_ms", "solve_ms", "total_ms"], out[56:60].tolist()))

    def sample(self, noise):
        e = _f64(noise).ravel()
        out = np.empty(e.size)
        _chk(lib().ck_sample(self._h, _p(e), _p(out), e.size))
        return out

    # -- step-wise form -----------------------------------------------------------------------
    def num_panels(self):
        n, w, npad = c_int(0), c_int(0), c_int64(0)
        _chk(lib().ck_num_panels(self._h, byref(n), byref(w), byref(npad)))
        return n.value, w.value, npad.value

    def panel_owner(self, K):
        o = c_int(0)
        _chk(lib().ck_panel_owner(self._h, int(K), byref(o)))
        return o.value

    def aux_begin(self, i, pcoords):
        pc = _f64(pcoords, 2)
        self._m = pc.shape[0]
        _chk(lib().ck_aux_begin(self._h, int(i), _p(pc), pc.shape[0]))

    def panel_factor(self, K):
        _chk(lib().ck_panel_factor(self._h, int(K)))

    def panel_buffer(self, K):
        p, nb = c_void_p(), c_int64(0)
        _chk(lib().ck_panel_buffer(self._h, int(K), byref(p), byref(nb)))
        return p.value, nb.value

    def panel_apply(self, K, what):
        _chk(lib().ck_panel_apply(self._h, int(K), int(what)))

    def panel_apply_sigma(self, K, J_lo, J_hi):
        _chk(lib().ck_panel_apply_sigma(self._h, int(K), int(J_lo), int(J_hi)))

    def panel_apply_group(self, K0, np_, what, J_lo, J_hi, phase=0, n_phase=1):
        _chk(lib().ck_panel_apply_group(self._h, int(K0), int(np_), int(what), int(J_lo), int(J_hi), int(phase), int(n_phase)))

    def panel_aux_solve(self, K):
        _chk(lib().ck_panel_aux_solve(self._h, int(K)))

    def aux_finish(self):
        pred, err = np.empty(self._m), np.empty(self._m)
        _chk(lib().ck_aux_finish(self._h, _p(pred), _p(err)))
        return pred, err

    def factor_info(self) -> int:
        info = c_int64(0)
        _chk(lib().ck_factor_info(self._h, byref(info)))
        return info.value

    # -- local-neighbourhood prediction ---------------------------------------------------------------
    def predict_local(self, i, pcoords, max_dist=1e3, cv=False):
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        pred, err = np.empty(m), np.empty(m)
        ne, npd, km = c_int64(0), c_int64(0), c_int64(0)
        _chk(lib().ck_predict_local(self._h, int(i), _p(pc), m, float(max_dist), int(bool(cv)), _p(pred), _p(err),
                                    byref(ne), byref(npd), byref(km)))
        return pred, err, dict(n_empty=ne.value, n_not_pd=npd.value, k_max=km.value)

    def predict_local_universal(self, i, pcoords, f0=None, max_dist=1e3, cv=False, want_beta=False):
        """Universal cokriging of process i in the moving neighbourhood, with the trend of set_trend (include/cokrige.h:
        ck_predict_local_universal).  f0: (m, p_i) regressors of process i at pcoords; a row with a non-finite entry gives
        NaN.  Returns (pred, err, info) with n_empty, n_not_pd, n_rank_def, k_max and, with ``want_beta``, beta (m, p): every
        site's local GLS coefficients.  Without a trend (p = 0) the predict_local result."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        p = sum(self._trend_p.values())
        pi = self._trend_p.get(int(i), 0)
        F0 = None
        if pi > 0:
            F0 = _f64(np.zeros((m, 0)) if f0 is None else f0)
            if F0.shape != (m, pi):
                raise ValueError(f"f0 has shape {F0.shape}, expected {(m, pi)}")
        pred, err = np.empty(m), np.empty(m)
        beta = np.full((m, p), np.nan) if want_beta else None
        ne, npd, nrd, km = c_int64(0), c_int64(0), c_int64(0), c_int64(0)
        _chk(lib().ck_predict_local_universal(self._h, int(i), _p(pc), m, _p(F0) if F0 is not None else None, float(max_dist),
                                              int(bool(cv)), _p(pred), _p(err), _p(beta) if want_beta and p else None,
                                              byref(ne), byref(npd), byref(nrd), byref(km)))
        info = dict(n_empty=ne.value, n_not_pd=npd.value, n_rank_def=nrd.value, k_max=km.value)
        if want_beta:
            info["beta"] = beta
        return pred, err, info

    def local_universal_timings(self):
        """ck_timings [48 ..] of the last predict_local_universal() call (milliseconds; the last two are counts)."""
        out = np.zeros(54)
        _chk(lib().ck_timings(self._h, _p(out), 54))
        keys = ["count_ms", "factor_ms", "reduce_ms", "total_ms", "n_lds", "n_tiled"]
        return dict(zip(keys, out[48:54].tolist()))

    def predict_local_blocks(self, i, centres, pcoords, block, weight, f0=None, max_dist=1e3, want_beta=False):
        """Block cokriging of process i in the moving neighbourhood (include/cokrige.h: ck_predict_local_blocks): the weighted
        means over the members of r = len(centres) blocks, each from the neighbourhood of its search centre.  block[a] in [0, r)
        names the block of member site a, weight[a] its weight; f0: (r, p_i) block regressors sum_a w_a f_i(x_a) under a trend.
        Returns (pred, err, info) like predict_local_universal, r values each.  No covariance between blocks exists here."""
        cc = _f64(centres, 2)
        pc = _f64(pcoords, 2)
        r, m = cc.shape[0], pc.shape[0]
        b = np.ascontiguousarray(block, dtype=np.int32).ravel()
        w = _f64(weight).ravel()
        if b.size != m or w.size != m:
            raise ValueError("pcoords, block and weight disagree in length")
        p = sum(self._trend_p.values())
        pi = self._trend_p.get(int(i), 0)
        F0 = None
        if pi > 0 and f0 is not None:   # a missing f0 is the library's refusal
            F0 = _f64(f0)
            if F0.shape != (r, pi):
                raise ValueError(f"f0 has shape {F0.shape}, expected {(r, pi)}")
        pred, err = np.empty(r), np.empty(r)
        beta = np.full((r, p), np.nan) if want_beta else None
        ne, npd, nrd, km = c_int64(0), c_int64(0), c_int64(0), c_int64(0)
        _chk(lib().ck_predict_local_blocks(self._h, int(i), _p(cc), r, _p(pc), m, b.ctypes.data_as(POINTER(c_int32)), _p(w),
                                           _p(F0) if F0 is not None else None, float(max_dist), _p(pred), _p(err),
                                           _p(beta) if want_beta and p else None, byref(ne), byref(npd), byref(nrd), byref(km)))
        info = dict(n_empty=ne.value, n_not_pd=npd.value, n_rank_def=nrd.value, k_max=km.value)
        if want_beta:
            info["beta"] = beta
        return pred, err, info

    def local_blocks_timings(self):
        """ck_timings [104 ..] of the last predict_local_blocks() call (milliseconds; the last is a count)."""
        out = np.zeros(110)
        _chk(lib().ck_timings(self._h, _p(out), 110))
        keys = ["count_ms", "lds_ms", "tiled_ms", "prior_ms", "total_ms", "cbar_evals"]
        return dict(zip(keys, out[104:110].tolist()))

    def predict_local_pair(self, pcoords, max_dist=1e3):
        """Both processes at every site from one local system (include/cokrige.h: ck_predict_local_pair): the neighbourhood,
        the local Sigma and its Cholesky are predict_local's (cv off) and serve both processes.  Returns (pred0, err0, pred1,
        err1, cov, info): cov the covariance of the two prediction errors at each site, info with n_empty, n_not_pd, k_max.
        pred / err carry the bits of predict_local(0) and predict_local(1).  No covariance between sites exists here."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        out = [np.empty(m) for _ in range(5)]
        ne, npd, km = c_int64(0), c_int64(0), c_int64(0)
        _chk(lib().ck_predict_local_pair(self._h, _p(pc), m, float(max_dist), *[_p(o) for o in out], byref(ne), byref(npd),
                                         byref(km)))
        return (*out, dict(n_empty=ne.value, n_not_pd=npd.value, k_max=km.value))

    def local_pair_timings(self):
        """ck_timings [138 ..] of the last predict_local_pair() call (milliseconds; the last two are counts)."""
        out = np.zeros(143)
        _chk(lib().ck_timings(self._h, _p(out), 143))
        keys = ["pass_ms", "solve_ms", "grow_ms", "n_tiled", "n_tiled_batches"]
        return dict(zip(keys, out[138:143].tolist()))

    def simulate_local(self, i, pcoords, rank, max_dist, n_draws, seed=0, noise=None, terms=True):
        """Draws of process i at pcoords by sequential simulation in the moving neighbourhood (include/cokrige.h:
        ck_simulate_local): site t is conditioned on the data and on the sites of smaller ``rank`` (m distinct integers) within
        ``max_dist``, under the caps of set_local_neighbours.  ``noise``: (n_draws, m) normals in the caller's order, else the
        device's Philox stream keyed on ``seed``.  Returns (draws (n_draws, m), info, stats): info = 1 + the first site whose
        local system is not positive definite or whose variance is not > 0 (its draws, and those of the sites that condition
        on it, are NaN), 0 otherwise; stats: n_empty, k_max, n_capped, n_levels and, with ``terms``, mean (mu_t^data), var
        (s_t^2) and count (m, 3: data of process 0, of process 1, earlier sites)."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        if r.size != m:
            raise ValueError(f"rank has {r.size} entries, pcoords {m} sites")
        n_draws = int(n_draws)
        e = None
        if noise is not None:
            e = _f64(noise)
            if e.shape != (n_draws, m):
                raise ValueError(f"noise has shape {e.shape}, expected {(n_draws, m)}")
        draws = np.zeros((max(n_draws, 0), m))
        mean = np.empty(m) if terms else None
        var = np.empty(m) if terms else None
        count = np.zeros((m, 3), dtype=np.int32) if terms else None
        st, info = np.zeros(4, dtype=np.int64), c_int64(0)
        _chk(lib().ck_simulate_local(self._h, int(i), _p(pc), m, r.ctypes.data_as(POINTER(c_int64)), float(max_dist), n_draws,
                                     c_uint64(int(seed) & (2 ** 64 - 1)), _p(e) if e is not None else None, _p(draws),
                                     _p(mean) if terms else None, _p(var) if terms else None,
                                     count.ctypes.data_as(POINTER(c_int32)) if terms else None,
                                     st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]), n_levels=int(st[3]))
        if terms:
            stats.update(mean=mean, var=var, count=count)
        return draws, info.value, stats

    def simulate_local_weights(self, i, pcoords, rank, max_dist):
        """(idx, w), both (m, 64): every site's conditioning set as stacked caller indices (data 0 .. N - 1, a site N + its
        index), ascending and padded with -1, and the weights w = Sigma_loc^-1 c in the same order (include/cokrige.h:
        ck_debug_simulate_local_weights)."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        if r.size != m:
            raise ValueError(f"rank has {r.size} entries, pcoords {m} sites")
        idx, w = np.full((m, 64), -1, dtype=np.int64), np.zeros((m, 64))
        _chk(lib().ck_debug_simulate_local_weights(self._h, int(i), _p(pc), m, r.ctypes.data_as(POINTER(c_int64)), float(max_dist),
                                                   idx.ctypes.data_as(POINTER(c_int64)), _p(w)))
        return idx, w

    def simulate_local_pair(self, pcoords0, pcoords1, rank, max_dist, n_draws, seed=0, noise=None, terms=True):
        """Sequential co-simulation of both processes in the moving neighbourhood (include/cokrige.h: ck_simulate_local_pair):
        process 0 at pcoords0 (m0 sites), process 1 at pcoords1 (m1), stacked -- index k for site k of process 0, m0 + k for
        site k of process 1.  ``rank``: m0 + m1 distinct integers over the stacked sites; a stacked site is conditioned on the
        data and on the stacked sites of smaller rank, of either process, within ``max_dist`` and under the caps.  ``noise``:
        (n_draws, m0 + m1), process 0's columns first.  Returns (draws (n_draws, m0 + m1), info, stats) as simulate_local;
        count has four columns (data of process 0, of process 1, earlier sites of process 0, of process 1)."""
        pc0, pc1 = _f64(np.zeros((0, 2)) if pcoords0 is None else pcoords0, 2), _f64(np.zeros((0, 2)) if pcoords1 is None else pcoords1, 2)
        m0, m1 = pc0.shape[0], pc1.shape[0]
        m = m0 + m1
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        if r.size != m:
            raise ValueError(f"rank has {r.size} entries, the two site sets {m} sites")
        n_draws = int(n_draws)
        e = None
        if noise is not None:
            e = _f64(noise)
            if e.shape != (n_draws, m):
                raise ValueError(f"noise has shape {e.shape}, expected {(n_draws, m)}")
        draws = np.zeros((max(n_draws, 0), m))
        mean = np.empty(m) if terms else None
        var = np.empty(m) if terms else None
        count = np.zeros((m, 4), dtype=np.int32) if terms else None
        st, info = np.zeros(4, dtype=np.int64), c_int64(0)
        _chk(lib().ck_simulate_local_pair(self._h, _p(pc0) if m0 else None, m0, _p(pc1) if m1 else None, m1,
                                          r.ctypes.data_as(POINTER(c_int64)), float(max_dist), n_draws,
                                          c_uint64(int(seed) & (2 ** 64 - 1)), _p(e) if e is not None else None, _p(draws),
                                          _p(mean) if terms else None, _p(var) if terms else None,
                                          count.ctypes.data_as(POINTER(c_int32)) if terms else None,
                                          st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]), n_levels=int(st[3]))
        if terms:
            stats.update(mean=mean, var=var, count=count)
        return draws, info.value, stats

    def simulate_local_pair_weights(self, pcoords0, pcoords1, rank, max_dist):
        """(idx, w), both (m0 + m1, 64): simulate_local_weights for the stacked sites of both processes -- a site is N + its
        stacked index (include/cokrige.h: ck_debug_simulate_local_pair_weights)."""
        pc0, pc1 = _f64(np.zeros((0, 2)) if pcoords0 is None else pcoords0, 2), _f64(np.zeros((0, 2)) if pcoords1 is None else pcoords1, 2)
        m0, m1 = pc0.shape[0], pc1.shape[0]
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        if r.size != m0 + m1:
            raise ValueError(f"rank has {r.size} entries, the two site sets {m0 + m1} sites")
        idx, w = np.full((m0 + m1, 64), -1, dtype=np.int64), np.zeros((m0 + m1, 64))
        _chk(lib().ck_debug_simulate_local_pair_weights(self._h, _p(pc0) if m0 else None, m0, _p(pc1) if m1 else None, m1,
                                                        r.ctypes.data_as(POINTER(c_int64)), float(max_dist),
                                                        idx.ctypes.data_as(POINTER(c_int64)), _p(w)))
        return idx, w

    def simulate_local_timings(self):
        """ck_timings [110 ..] of the last simulate_local() call (milliseconds; the last three are counts)."""
        out = np.zeros(118)
        _chk(lib().ck_timings(self._h, _p(out), 118))
        keys = ["select_ms", "weights_ms", "levels_ms", "recursion_ms", "total_ms", "n_solved", "n_levels", "n_site_neighbours"]
        return dict(zip(keys, out[110:118].tolist()))

    def set_local_neighbours(self, n0: int, n1: int = 0):
        """Nearest-neighbour cap per process of the local predictor (include/cokrige.h: ck_set_local_neighbours); 0 = none."""
        _chk(lib().ck_set_local_neighbours(self._h, int(n0), int(n1)))

    def local_neighbours(self, i, pcoords, max_dist=1e3, cv=False):
        """(count, rcut), both (m, 2): per point and process the number of neighbours under the handle's caps and the cut
        distance r_pq (include/cokrige.h: ck_debug_local_neighbours)."""
        pc = _f64(pcoords, 2)
        m = pc.shape[0]
        count, rcut = np.zeros((m, 2), dtype=np.int32), np.zeros((m, 2))
        _chk(lib().ck_debug_local_neighbours(self._h, int(i), _p(pc), m, float(max_dist), int(bool(cv)),
                                             count.ctypes.data_as(POINTER(c_int32)), _p(rcut)))
        return count, rcut

    def _cv_local_args(self, i, folds_i, folds_other, n_folds, buffer):
        """(n_i, fold0, fold1, n_folds, buffer2, keepalive) of the two cross-validation calls of the local predictor"""
        i = int(i)
        n_i = int(self._n_data.get(i, 0))
        ip = POINTER(c_int32)
        fi = None if folds_i is None else np.ascontiguousarray(folds_i, dtype=np.int32).ravel()
        fo = None if folds_other is None else np.ascontiguousarray(folds_other, dtype=np.int32).ravel()
        if fi is not None and fi.size != n_i:
            raise ValueError(f"folds_i has {fi.size} labels, process {i} has {n_i} data")
        n_o = int(self._n_data.get(1 - i, 0))
        if fo is not None and fo.size != n_o:
            raise ValueError(f"folds_other has {fo.size} labels, process {1 - i} has {n_o} data")
        if n_folds is None:
            n_folds = int(max(-1 if fi is None else fi.max(initial=-1), -1 if fo is None else fo.max(initial=-1))) + 1
        pi = None if fi is None else fi.ctypes.data_as(ip)
        po = None if fo is None else fo.ctypes.data_as(ip)
        f0, f1 = (pi, po) if i == 0 else (po, pi)
        b2 = None
        if buffer is not None:
            b = [buffer, buffer] if np.isscalar(buffer) else list(buffer)
            if len(b) != 2:
                raise ValueError("buffer is a number or one entry per process (None = off)")
            b2 = np.array([-1.0 if x is None else float(x) for x in b], dtype=np.float64)
        return n_i, f0, f1, int(n_folds), b2, (fi, fo)

    def cv_local_folds(self, i, folds_i=None, folds_other=None, n_folds=None, buffer=None, f0=None, max_dist=1e3, want_beta=False):
        """Leave-group-out / buffer cross-validation of process ``i`` in the moving neighbourhood (include/cokrige.h:
        ck_cv_local_folds).  ``folds_i`` / ``folds_other``: int labels in [-1, n_folds) of the data of process i / of the other
        process, the caller's order (-1 = never withheld; None: no labels).  ``buffer``: None, a radius for both processes, or a pair
        (an entry of None or < 0: off).  ``f0``: (n_i, p_i) regressors at the data of process i when a trend is set.
        Returns (pred, pred_err, info): n_empty, n_not_pd, n_rank_def, k_max, fold_stats (n_folds, 6), score5 and, with
        ``want_beta``, beta (n_i, p)."""
        n_i, p0, p1, n_folds, b2, keep = self._cv_local_args(i, folds_i, folds_other, n_folds, buffer)
        p = sum(self._trend_p.values())
        pi = self._trend_p.get(int(i), 0)
        F0 = None
        if pi > 0:
            F0 = _f64(np.zeros((n_i, 0)) if f0 is None else f0)
            if F0.shape != (n_i, pi):
                raise ValueError(f"f0 has shape {F0.shape}, expected {(n_i, pi)}")
        pred, err = np.empty(n_i), np.empty(n_i)
        beta = np.full((n_i, p), np.nan) if want_beta else None
        stats, score = np.zeros((max(n_folds, 0), 6)), np.zeros(5)
        cnt = np.zeros(4, dtype=np.int64)
        _chk(lib().ck_cv_local_folds(self._h, int(i), p0, p1, n_folds, None if b2 is None else _p(b2), _p(F0) if F0 is not None else None,
                                     float(max_dist), _p(pred), _p(err), _p(beta) if want_beta and p else None, _p(stats), _p(score),
                                     cnt.ctypes.data_as(POINTER(c_int64))))
        info = dict(n_empty=int(cnt[0]), n_not_pd=int(cnt[1]), n_rank_def=int(cnt[2]), k_max=int(cnt[3]), fold_stats=stats, score5=score)
        if want_beta:
            info["beta"] = beta
        return pred, err, info

    def local_cv_neighbours(self, i, folds_i=None, folds_other=None, n_folds=None, buffer=None, max_dist=1e3):
        """(count, rcut), both (n_i, 2): the select pass of cv_local_folds alone (include/cokrige.h: ck_debug_local_cv_neighbours);
        (0, NaN) rows for data that are never withheld."""
        n_i, p0, p1, n_folds, b2, keep = self._cv_local_args(i, folds_i, folds_other, n_folds, buffer)
        count, rcut = np.zeros((n_i, 2), dtype=np.int32), np.zeros((n_i, 2))
        _chk(lib().ck_debug_local_cv_neighbours(self._h, int(i), p0, p1, n_folds, None if b2 is None else _p(b2), float(max_dist),
                                                count.ctypes.data_as(POINTER(c_int32)), _p(rcut)))
        return count, rcut

    def cv_local_timings(self):
        """ck_timings [118 ..] of the last cv_local_folds() call (milliseconds; the last two are counts)."""
        out = np.zeros(124)
        _chk(lib().ck_timings(self._h, _p(out), 124))
        keys = ["pass_ms", "solve_ms", "scores_ms", "total_ms", "n_predicted", "n_folds"]
        return dict(zip(keys, out[118:124].tolist()))

    def loglik_vecchia(self, rank, max_dist, terms=False):
        """Vecchia log-likelihood of the data under the model (include/cokrige.h: ck_loglik_vecchia): every datum conditioned on
        the data of smaller ``rank`` (N distinct integers, stacked: process 0 then 1) within ``max_dist``, under the caps of
        set_local_neighbours.  Returns (out3, info, stats) -- out3 = (l, sum log s_t^2, sum e_t^2 / s_t^2), NaN with info =
        1 + the first datum without a term; stats: n_empty, k_max, n_capped -- and with ``terms`` also mean, var (N) and
        count (N, 2) in stats."""
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        n = int(sum(self._n_data.values()))
        if r.size != n:
            raise ValueError(f"rank has {r.size} entries, the handle {n} data")
        out3, st, info = np.zeros(3), np.zeros(3, dtype=np.int64), c_int64(0)
        mean = np.empty(n) if terms else None
        var = np.empty(n) if terms else None
        count = np.zeros((n, 2), dtype=np.int32) if terms else None
        _chk(lib().ck_loglik_vecchia(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist), _p(out3),
                                     _p(mean) if terms else None, _p(var) if terms else None,
                                     count.ctypes.data_as(POINTER(c_int32)) if terms else None,
                                     st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]))
        if terms:
            stats.update(mean=mean, var=var, count=count)
        return out3, info.value, stats

    def vecchia_timings(self):
        """ck_timings [72 ..] of the last loglik_vecchia() call (milliseconds; the last two are counts of data)."""
        out = np.zeros(78)
        _chk(lib().ck_timings(self._h, _p(out), 78))
        keys = ["select_ms", "solve_ms", "terms_ms", "total_ms", "n_lds", "n_tiled"]
        return dict(zip(keys, out[72:78].tolist()))

    def loglik_vecchia_grad(self, rank, max_dist, free=None, scores=False):
        """Vecchia log-likelihood with its analytic gradient (include/cokrige.h: ck_loglik_vecchia_grad), for conditioning sets
        of at most 64 data.  ``free``: 13 flags over the slots of fisher() (None: all).  Returns (out3, grad13, info, stats):
        out3 has loglik_vecchia's bits; grad13 holds exact zeros in the slots that are not live and is NaN when info != 0;
        with ``scores`` stats["score"] is the (N, 13) array of the per-datum contributions in the stacked order."""
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        n = int(sum(self._n_data.values()))
        if r.size != n:
            raise ValueError(f"rank has {r.size} entries, the handle {n} data")
        fr = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free).astype(bool), dtype=np.int32)
            if fr.shape != (13,):
                raise ValueError("free: 13 flags, one per slot")
        out3, grad, st, info = np.zeros(3), np.zeros(13), np.zeros(3, dtype=np.int64), c_int64(0)
        score = np.empty((n, 13)) if scores else None
        _chk(lib().ck_loglik_vecchia_grad(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist),
                                          fr.ctypes.data_as(POINTER(c_int32)) if fr is not None else None, _p(out3), _p(grad),
                                          _p(score) if scores else None, st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]))
        if scores:
            stats["score"] = score
        return out3, grad, info.value, stats

    def vecchia_grad_timings(self):
        """ck_timings [80 ..] of the last loglik_vecchia_grad() call (milliseconds; the last two are counts)."""
        out = np.zeros(86)
        _chk(lib().ck_timings(self._h, _p(out), 86))
        keys = ["select_ms", "solve_ms", "reduce_ms", "total_ms", "n_data", "n_pairs"]
        return dict(zip(keys, out[80:86].tolist()))

    def loglik_vecchia_fisher(self, rank, max_dist, free=None):
        """Expected information of the Vecchia likelihood (include/cokrige.h: ck_loglik_vecchia_fisher), for conditioning sets
        of at most 64 data, on the sets loglik_vecchia uses.  ``free``: 13 flags over the slots of fisher() (None: all).
        Returns (fisher, info, stats): the 13 x 13 array, symmetric, exact zeros in the rows and columns of slots that are not
        live; info = 1 + the first datum without a term (the live block is then NaN), else 0; stats: n_empty, k_max, n_capped."""
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        n = int(sum(self._n_data.values()))
        if r.size != n:
            raise ValueError(f"rank has {r.size} entries, the handle {n} data")
        fr = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free).astype(bool), dtype=np.int32)
            if fr.shape != (13,):
                raise ValueError("free: 13 flags, one per slot")
        out, st, info = np.empty((13, 13)), np.zeros(3, dtype=np.int64), c_int64(0)
        _chk(lib().ck_loglik_vecchia_fisher(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist),
                                            fr.ctypes.data_as(POINTER(c_int32)) if fr is not None else None, _p(out),
                                            st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        return out, info.value, dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]))

    def vecchia_fisher_timings(self):
        """ck_timings [88 ..] of the last loglik_vecchia_fisher() call (milliseconds; the last two are counts)."""
        out = np.zeros(94)
        _chk(lib().ck_timings(self._h, _p(out), 94))
        keys = ["select_ms", "kernel_ms", "reduce_ms", "total_ms", "n_data", "n_entries"]
        return dict(zip(keys, out[88:94].tolist()))

    def _ranks_arg(self, rank):
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        n = int(sum(self._n_data.values()))
        if r.size != n:
            raise ValueError(f"rank has {r.size} entries, the handle {n} data")
        return r, n

    def loglik_vecchia_trend(self, rank, max_dist, reml=False, terms=False):
        """Vecchia log-likelihood with the trend of set_trend estimated by GLS inside it (include/cokrige.h:
        ck_loglik_vecchia_trend): the profile value, or with ``reml`` the restricted one, for conditioning sets of at most 64
        data.  Returns (out5, beta, beta_cov, info, stats): out5 = (l, sum log s_t^2, log|A|, Q, yy); beta (p) and beta_cov
        (p, p) over the trend columns of both processes; all NaN with info = 1 + the first datum without a term; stats as
        loglik_vecchia (with ``terms`` the mean under the fitted trend, var and count).  Without a trend it is loglik_vecchia."""
        r, n = self._ranks_arg(rank)
        p = sum(self._trend_p.values())
        out5, st, info = np.zeros(5), np.zeros(3, dtype=np.int64), c_int64(0)
        beta, cov = np.zeros(p), np.zeros((p, p))
        mean = np.empty(n) if terms else None
        var = np.empty(n) if terms else None
        count = np.zeros((n, 2), dtype=np.int32) if terms else None
        _chk(lib().ck_loglik_vecchia_trend(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist), int(bool(reml)), _p(out5),
                                           _p(beta) if p else None, _p(cov) if p else None,
                                           _p(mean) if terms else None, _p(var) if terms else None,
                                           count.ctypes.data_as(POINTER(c_int32)) if terms else None,
                                           st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]))
        if terms:
            stats.update(mean=mean, var=var, count=count)
        return out5, beta, cov, info.value, stats

    def loglik_vecchia_trend_grad(self, rank, max_dist, free=None, scores=False):
        """The profile value of loglik_vecchia_trend with its analytic gradient at beta-hat (include/cokrige.h:
        ck_loglik_vecchia_trend_grad).  Returns (out5, beta, beta_cov, grad13, info, stats): out5 and beta have the value call's
        bits; grad13, ``free`` and ``scores`` as loglik_vecchia_grad."""
        r, n = self._ranks_arg(rank)
        p = sum(self._trend_p.values())
        fr = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free).astype(bool), dtype=np.int32)
            if fr.shape != (13,):
                raise ValueError("free: 13 flags, one per slot")
        out5, grad, st, info = np.zeros(5), np.zeros(13), np.zeros(3, dtype=np.int64), c_int64(0)
        beta, cov = np.zeros(p), np.zeros((p, p))
        score = np.empty((n, 13)) if scores else None
        _chk(lib().ck_loglik_vecchia_trend_grad(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist),
                                                fr.ctypes.data_as(POINTER(c_int32)) if fr is not None else None, _p(out5),
                                                _p(beta) if p else None, _p(cov) if p else None, _p(grad),
                                                _p(score) if scores else None, st.ctypes.data_as(POINTER(c_int64)), byref(info)))
        stats = dict(n_empty=int(st[0]), k_max=int(st[1]), n_capped=int(st[2]))
        if scores:
            stats["score"] = score
        return out5, beta, cov, grad, info.value, stats

    def debug_vecchia_trend(self, rank, max_dist):
        """(mu, vv, g) of every datum's local solve with the trend rows riding along (include/cokrige.h: ck_debug_vecchia_trend):
        v . y, v . v (N each) and U^T v (N, p) in the stacked order."""
        r, n = self._ranks_arg(rank)
        p = sum(self._trend_p.values())
        mu, vv, g = np.empty(n), np.empty(n), np.zeros((n, max(p, 1)))
        _chk(lib().ck_debug_vecchia_trend(self._h, r.ctypes.data_as(POINTER(c_int64)), float(max_dist), _p(mu), _p(vv), _p(g)))
        return mu, vv, g[:, :p] if p else np.zeros((n, 0))

    def vecchia_trend_timings(self):
        """ck_timings [96 ..] of the last loglik_vecchia_trend() / _trend_grad() call (milliseconds; the last two are counts)."""
        out = np.zeros(103)
        _chk(lib().ck_timings(self._h, _p(out), 103))
        keys = ["select_ms", "solve_ms", "terms_gram_ms", "grad_ms", "total_ms", "n_data", "p"]
        return dict(zip(keys, out[96:103].tolist()))

    def local_reserve(self, nbytes: int = 0):
        """Pre-size the scratch slab of predict_local (0: the automatic budget) -- include/cokrige.h: ck_local_reserve."""
        _chk(lib().ck_local_reserve(self._h, int(nbytes)))

    # -- empirical variogram ------------------------------------------------------------------------
    def vario_begin(self, coords_i, resid_i, coords_j=None, resid_j=None):
        ci, ri = _f64(coords_i, 2), _f64(resid_i).ravel()
        if coords_j is None:
            _chk(lib().ck_vario_begin(self._h, _p(ci), _p(ri), ci.shape[0], None, None, 0, 1))
        else:
            cj, rj = _f64(coords_j, 2), _f64(resid_j).ravel()
            _chk(lib().ck_vario_begin(self._h, _p(ci), _p(ri), ci.shape[0], _p(cj), _p(rj), cj.shape[0], 0))

    def vario_extent(self, max_dist):
        lo, hi, npos = c_double(0), c_double(0), c_int64(0)
        _chk(lib().ck_vario_extent(self._h, float(max_dist), byref(lo), byref(hi), byref(npos)))
        return lo.value, hi.value, npos.value

    def vario_bin(self, max_dist, edges, covariogram=False):
        e = _f64(edges).ravel()
        nb = e.size - 1
        sums = np.empty(nb)
        counts = np.empty(nb, dtype=np.int64)
        _chk(lib().ck_vario_bin(self._h, float(max_dist), _p(e), e.size, int(bool(covariogram)), _p(sums),
                                counts.ctypes.data_as(POINTER(c_int64))))
        return sums, counts

    def vario_end(self):
        _chk(lib().ck_vario_end(self._h))

    def vario_stats(self):
        out = np.zeros(4, dtype=np.int64)
        _chk(lib().ck_vario_stats(self._h, out.ctypes.data_as(POINTER(c_int64)), 4))
        return dict(zip(["extent_host_pairs", "bin_host_pairs", "bin_visited_pairs", "extent_extra_rounds"], out.tolist()))

    # -- diagnostics -----------------------------------------------------------------------------
    def debug_matern_grad(self, block, h):
        """(n, 3): (M, dM/dnu, dM/dlen) of the Matern correlation of block `block` at the lags h, as the likelihood kernels
        evaluate them per entry (include/cokrige.h: ck_debug_matern_grad)."""
        h = _f64(h).ravel()
        out = np.empty((h.size, 3))
        _chk(lib().ck_debug_matern_grad(self._h, int(block), _p(h), h.size, _p(out)))
        return out

    def debug_get_lower(self, n):
        out = np.empty((n, n))
        _chk(lib().ck_debug_get_lower(self._h, _p(out), int(n)))
        return out

    def debug_get_entries(self, rows, cols):
        """Sigma[rows[e], cols[e]] (after assemble_joint) or L[max, min] (after factor); caller's stacked site order."""
        r = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        c = np.ascontiguousarray(cols, dtype=np.int64).ravel()
        if r.size != c.size:
            raise ValueError("rows and cols disagree in length")
        out = np.empty(r.size)
        _chk(lib().ck_debug_get_entries(self._h, r.ctypes.data_as(POINTER(c_int64)), c.ctypes.data_as(POINTER(c_int64)), r.size,
                                        _p(out)))
        return out

    def debug_site_order(self, k, n_k):
        """perm[j] = caller's index (within process k) of the site at internal position j."""
        out = np.empty(int(n_k), dtype=np.int64)
        _chk(lib().ck_debug_site_order(self._h, int(k), out.ctypes.data_as(POINTER(c_int64)), int(n_k)))
        return out

    def potrf_profile(self, iters=200):
        out = np.zeros(8)
        _chk(lib().ck_debug_potrf_profile(self._h, int(iters), _p(out)))
        keys = ["load_us", "factor_us", "scale_store_us", "inv_diag_us", "inv_offdiag_us", "inv_store_us", "launch_prof_us",
                "launch_us"]
        return dict(zip(keys, out.tolist()))

    def coop_profile(self, rows=4096):
        out = np.zeros(64)
        _chk(lib().ck_debug_coop_profile(self._h, int(rows), _p(out)))
        return out

    def mfma_probe(self):
        out = np.empty(64 * 4 * 3, dtype=np.int32)
        _chk(lib().ck_debug_mfma_probe(self._h, out.ctypes.data_as(POINTER(c_int32))))
        return out.reshape(64, 4, 3)

    def table_info(self, block):
        en, ni = c_int(0), c_int(0)
        ql, qh, er = c_double(0), c_double(0), c_double(0)
        _chk(lib().ck_table_info(self._h, int(block), byref(en), byref(ni), byref(ql), byref(qh), byref(er)))
        return dict(enabled=bool(en.value), n_intervals=ni.value, q_lo=ql.value, q_hi=qh.value,
                    max_rel_err=er.value)

    def table_fallbacks(self, reset=True):
        c = c_int64(0)
        _chk(lib().ck_table_fallbacks(self._h, int(bool(reset)), byref(c)))
        return c.value

    def cu_probe(self, mask_words=None, n_wg=4096):
        """(xcc, se, sh, cu) of each workgroup of a launch on a CU-masked stream (None: unmasked)."""
        out = np.zeros(int(n_wg), dtype=np.uint32)
        mp = None
        if mask_words is not None:
            mk = np.ascontiguousarray(mask_words, dtype=np.uint32)
            assert mk.size == 8
            mp = mk.ctypes.data_as(POINTER(c_uint32))
        _chk(lib().ck_debug_cu_probe(self._h, mp, int(n_wg), out.ctypes.data_as(POINTER(c_uint32))))
        return np.stack([out >> 16, (out >> 8) & 7, (out >> 4) & 1, out & 15], axis=1)

    def mfma_peak(self, waves_per_simd=1, iters=20000):
        out = np.zeros(3)
        _chk(lib().ck_debug_mfma_peak(self._h, int(waves_per_simd), int(iters), _p(out)))
        return dict(tflops=out[0], shader_mhz=out[1], cycles_per_mfma_per_wave=out[2])

    def gemm_clock(self):
        """After set_option("gemm_stamps", 1) and a factorisation: the in-kernel clock of the trailing updates."""
        out = np.zeros(6)
        _chk(lib().ck_debug_gemm_clock(self._h, _p(out)))
        return dict(mhz_median=out[0], mhz_p05=out[1], mhz_p95=out[2], workgroups=int(out[3]),
                    wg_cycles_median=out[4], wg_us_median=out[5])

    def stream_overlap(self, mode, rows, n_side):
        out = np.zeros(1 + int(n_side))
        _chk(lib().ck_debug_stream_overlap(self._h, int(mode), int(rows), int(n_side), _p(out)))
        return out

    def gemm_stamps(self, n_workgroups):
        """Raw workgroup stamps of the last stamped trailing update: (n, 4) uint64 and (grid x, grid y, J0, panels)."""
        out = np.zeros((int(n_workgroups), 4), dtype=np.uint64)
        grid = np.zeros(4, dtype=np.int64)
        _chk(lib().ck_debug_gemm_stamps(self._h, out.ctypes.data_as(POINTER(c_uint64)), out.size,
                                        grid.ctypes.data_as(POINTER(c_int64))))
        return out, grid

    def timings(self):
        out = np.zeros(64)
        _chk(lib().ck_timings(self._h, _p(out), 64))
        # the neighbour cap of the local predictor (ck_set_local_neighbours): slots [60 ..]
        out = np.concatenate([out[:23], out[60:64]])
        keys = ["assemble_sigma_ms", "factor_ms", "assemble_aux_ms", "solve_ms", "reduce_ms", "syrk_ms",
                "syrk_launches", "aux_gemm_ms", "aux_gemm_launches", "vario_bin_ms", "local_ms", "verify_ms",
                "panel_coop_redone", "fused_sweeps_ms", "local_alloc_ms", "tall_union_ms",
                # ck_predict_blocks
                "blocks_assemble_ms", "blocks_fold_ms", "blocks_prior_ms", "blocks_solve_ms", "blocks_reduce_ms",
                "blocks_total_ms", "blocks_chunks",
                "local_select_ms", "local_n_capped", "local_cand_max", "local_n_rescan"]
        return dict(zip(keys, out.tolist()))

    def dev_gemm_nt(self, C_ptr, ldc, A_ptr, lda, B_ptr, ldb, M, N, K, lower=False):
        _chk(lib().ck_dev_gemm_nt(self._h, c_void_p(C_ptr), ldc, c_void_p(A_ptr), lda, c_void_p(B_ptr), ldb, M, N, K,
                                  int(bool(lower))))
