"""ctypes binding of libllpf_hip.so — one Python function per symbol of include/llpf.h.

This is the same binding a Julia maintainer writes with `ccall` (see INTEGRATION.md and
julia/LLPFAmd.jl); the tests drive the library through it.  There is no fallback: if the
shared library is missing or no GPU is visible, loading / constructing raises.
"""
import ctypes as C
import os

import numpy as np

from . import _structs as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LLPF_LIB") or os.path.join(_HERE, "libllpf_hip.so")   # LLPF_LIB: A/B builds of the same engine (tools/)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_vp = C.c_void_p

# every exported symbol of include/llpf.h with its argument types (restype is int unless noted)
SYMBOLS = {
    "llpf_create": [C.POINTER(S.Config), C.POINTER(_vp)],
    "llpf_destroy": [_vp],
    "llpf_reset": [_vp],
    "llpf_seed": [_vp, C.c_uint64],
    "llpf_set_model": [_vp, _vp],
    "llpf_correct": [_vp, _dp, _dp, C.c_double, _dp],
    "llpf_predict": [_vp, _dp, C.c_double],
    "llpf_update": [_vp, _dp, _dp, C.c_double, _dp],
    "llpf_run": [_vp, _dp, _dp, C.c_int64, C.c_double, _dp, C.POINTER(S.RunOutputs)],
    "llpf_smooth": [_vp, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, _dp, _ip],
    "llpf_rb_get_covariance": [_vp, _dp],
    "llpf_rb_get_linear_state": [_vp, _dp, _dp],
    "llpf_aux_correct": [_vp, _dp],
    "llpf_aux_predict": [_vp, _dp, _dp, C.c_double],
    "llpf_aux_update": [_vp, _dp, _dp, C.c_double, _dp],
    "llpf_aux_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(S.RunOutputs)],
    "llpf_bank_aux_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, _dp],
    "llpf_simulate": [_vp, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_double, C.c_uint64, C.c_uint32, C.c_int32, _dp, _dp],
    "llpf_bank_simulate": [_vp, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_double, C.c_uint64, C.c_uint32, C.c_int32, _dp, _dp],
    "llpf_kalman_bank_create": [C.c_int32, C.POINTER(S.Model), _dp, C.c_int32, C.POINTER(_vp)],
    "llpf_kalman_bank_destroy": [_vp],
    "llpf_kalman_bank_reset": [_vp],
    "llpf_kalman_bank_set_models": [_vp, C.POINTER(S.Model), _dp],
    "llpf_kalman_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_kalman_bank_smooth": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(S.KalmanOutputs), C.POINTER(S.KalmanSmoothOutputs)],
    "llpf_kalman_bank_get_state": [_vp, _dp, _dp],
    "llpf_kalman_bank_set_state": [_vp, _dp, _dp],
    "llpf_sqkf_bank_create": [C.c_int32, C.POINTER(S.Model), _dp, C.c_int32, C.POINTER(_vp)],
    "llpf_sqkf_bank_destroy": [_vp],
    "llpf_sqkf_bank_reset": [_vp],
    "llpf_sqkf_bank_set_models": [_vp, C.POINTER(S.Model), _dp],
    "llpf_sqkf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_sqkf_bank_get_state": [_vp, _dp, _dp, _dp],
    "llpf_sqkf_bank_set_state": [_vp, _dp, _dp, _dp],
    "llpf_imm_bank_create": [C.c_int32, C.POINTER(S.Model), _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)],
    "llpf_imm_bank_create_unscented": [C.c_int32, C.POINTER(S.Model), _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(S.UkfWeights), C.POINTER(_vp)],
    "llpf_imm_bank_set_weights": [_vp, C.POINTER(S.UkfWeights)],
    "llpf_imm_bank_destroy": [_vp],
    "llpf_imm_bank_reset": [_vp],
    "llpf_imm_bank_set_models": [_vp, C.POINTER(S.Model), _dp, _dp, _dp],
    "llpf_imm_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(S.ImmOutputs)],
    "llpf_imm_bank_run_at": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.ImmOutputs)],
    "llpf_imm_bank_get_state": [_vp, _dp, _dp, _dp, _dp, _dp],
    "llpf_imm_bank_set_state": [_vp, _dp, _dp, _dp],
    "llpf_ukf_bank_create": [C.c_int32, C.POINTER(S.Model), C.c_int32, C.POINTER(S.UkfWeights), C.POINTER(_vp)],
    "llpf_ukf_bank_destroy": [_vp],
    "llpf_ukf_bank_reset": [_vp],
    "llpf_ukf_bank_set_models": [_vp, C.POINTER(S.Model)],
    "llpf_ukf_bank_set_weights": [_vp, C.POINTER(S.UkfWeights)],
    "llpf_ukf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_ukf_bank_smooth": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs), C.POINTER(S.KalmanSmoothOutputs)],
    "llpf_ukf_bank_get_state": [_vp, _dp, _dp],
    "llpf_ukf_bank_set_state": [_vp, _dp, _dp],
    "llpf_aukf_bank_create": [C.c_int32, C.POINTER(S.Model), C.c_int32, C.POINTER(S.UkfWeights), C.POINTER(S.UkfWeights), C.POINTER(_vp)],
    "llpf_aukf_bank_destroy": [_vp],
    "llpf_aukf_bank_reset": [_vp],
    "llpf_aukf_bank_set_models": [_vp, C.POINTER(S.Model)],
    "llpf_aukf_bank_set_weights": [_vp, C.POINTER(S.UkfWeights), C.POINTER(S.UkfWeights)],
    "llpf_aukf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_aukf_bank_get_state": [_vp, _dp, _dp],
    "llpf_aukf_bank_set_state": [_vp, _dp, _dp],
    "llpf_ekf_bank_create": [C.c_int32, C.POINTER(S.Model), C.c_int32, C.POINTER(_vp)],
    "llpf_ekf_bank_destroy": [_vp],
    "llpf_ekf_bank_reset": [_vp],
    "llpf_ekf_bank_set_models": [_vp, C.POINTER(S.Model)],
    "llpf_ekf_bank_set_iterations": [_vp, C.c_int32, C.c_double],
    "llpf_ekf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_ekf_bank_get_state": [_vp, _dp, _dp],
    "llpf_ekf_bank_set_state": [_vp, _dp, _dp],
    "llpf_sqekf_bank_create": [C.c_int32, C.POINTER(S.Model), C.c_int32, C.POINTER(_vp)],
    "llpf_sqekf_bank_destroy": [_vp],
    "llpf_sqekf_bank_reset": [_vp],
    "llpf_sqekf_bank_set_models": [_vp, C.POINTER(S.Model)],
    "llpf_sqekf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_sqekf_bank_get_state": [_vp, _dp, _dp, _dp],
    "llpf_sqekf_bank_set_state": [_vp, _dp, _dp, _dp],
    "llpf_enkf_bank_create": [C.c_int32, C.POINTER(S.Model), C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)],
    "llpf_enkf_bank_destroy": [_vp],
    "llpf_enkf_bank_reset": [_vp],
    "llpf_enkf_bank_seed": [_vp, C.c_uint64],
    "llpf_enkf_bank_set_models": [_vp, C.POINTER(S.Model)],
    "llpf_enkf_bank_set_inflation": [_vp, C.c_double],
    "llpf_enkf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, C.c_double, _dp, C.POINTER(S.KalmanOutputs)],
    "llpf_enkf_bank_correct": [_vp, _dp, _dp, C.c_int32, C.c_double, _dp, _dp],
    "llpf_enkf_bank_predict": [_vp, _dp, C.c_int32, C.c_double],
    "llpf_enkf_bank_get_state": [_vp, _dp, _dp],
    "llpf_enkf_bank_get_members": [_vp, _dp],
    "llpf_enkf_bank_set_members": [_vp, _dp],
    "llpf_num_particles": [_vp, _ip],
    "llpf_index": [_vp, _ip],
    "llpf_get_particles": [_vp, _dp],
    "llpf_get_weights": [_vp, _dp],
    "llpf_get_expweights": [_vp, _dp],
    "llpf_get_ancestors": [_vp, _ip],
    "llpf_get_bins": [_vp, _dp],
    "llpf_set_particles": [_vp, _dp],
    "llpf_set_weights": [_vp, _dp],
    "llpf_set_index": [_vp, C.c_int64],
    "llpf_effective_particles": [_vp, _dp],
    "llpf_shouldresample": [_vp, C.POINTER(C.c_int32)],
    "llpf_weighted_mean": [_vp, _dp],
    "llpf_last_resampled": [_vp, C.POINTER(C.c_int32)],
    "llpf_maxw": [_vp, _dp],
    "llpf_logsumexp": [C.c_int32, _dp, _dp, C.c_int64, _dp],
    "llpf_resample": [C.c_int32, C.c_int32, _dp, C.c_int64, C.c_int64, _dp, _ip],
    "llpf_resample_uniforms": [C.c_int32, C.c_int64, C.c_uint64, C.c_uint32, _dp],
    "llpf_bank_create": [C.POINTER(S.Config), C.POINTER(S.Model), C.c_int32, C.POINTER(_vp)],
    "llpf_bank_destroy": [_vp],
    "llpf_bank_reset": [_vp],
    "llpf_bank_seed": [_vp, C.c_uint64],
    "llpf_bank_set_models": [_vp, _vp],
    "llpf_bank_run": [_vp, _dp, _dp, C.c_int64, C.c_double, _dp, _dp],
    "llpf_bank_run_multi": [_vp, _dp, _dp, C.c_int64, C.c_double, _dp, _dp, _dp],
    "llpf_mbank_create": [C.POINTER(S.Config), C.POINTER(S.Model), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(_vp)],
    "llpf_mbank_unique_id": [C.POINTER(C.c_uint8)],
    "llpf_mbank_partition": [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "llpf_mbank_create_rank": [C.POINTER(S.Config), C.POINTER(S.Model), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(_vp)],
    "llpf_mbank_destroy": [_vp],
    "llpf_mbank_reset": [_vp],
    "llpf_mbank_seed": [_vp, C.c_uint64],
    "llpf_mbank_set_models": [_vp, _vp],
    "llpf_mbank_run": [_vp, _dp, _dp, C.c_int64, C.c_double, _dp, _dp],
    "llpf_mbank_aux_run": [_vp, _dp, _dp, C.c_int64, C.c_int32, _dp, _dp],
    "llpf_mbank_info": [_vp, C.POINTER(S.MBankInfo)],
    "llpf_mbank_local_devices": [_vp, C.POINTER(C.c_int32)],
    "llpf_mbank_set_profiling": [_vp, C.c_int32],
    "llpf_mbank_get_profile": [_vp, C.c_int32, _dp, _ip],
    "llpf_model_compile": [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)],
    "llpf_model_traits": [C.c_int32, C.POINTER(C.c_int32)],
    "llpf_weighted_cov": [_vp, _dp],
    "llpf_weighted_quantile": [_vp, _dp, C.c_int32, _dp],
    "llpf_set_profiling": [_vp, C.c_int32],
    "llpf_get_profile": [_vp, _dp, _ip],
    "llpf_bank_set_profiling": [_vp, C.c_int32],
    "llpf_bank_get_profile": [_vp, _dp, _ip],
    "llpf_resample_count": [_vp, _ip],
    "llpf_bank_resample_count": [_vp, _ip],
    "llpf_last_run_ms": [_vp, _dp],
    "llpf_last_run_stats": [_vp, _ip, _ip, _dp],
    "llpf_last_run_form": [_vp, C.POINTER(C.c_int32), _ip],
    "llpf_bank_last_run_ms": [_vp, _dp],
    "llpf_last_error": [],
    "llpf_version": [C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "llpf_device_count": [C.POINTER(C.c_int32)],
    "llpf_selftest_math": [C.c_int32, C.c_int32, _dp, _dp, C.c_int64],
    "llpf_selftest_normals": [C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, _dp, C.c_int64],
}

SIM_DYNAMICS_NOISE, SIM_MEASUREMENT_NOISE, SIM_SAMPLE_INITIAL = 1, 2, 4
OK, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_DEGENERATE, ERR_ALLOC, ERR_INTERNAL = 0, 1, 2, 3, 4, 5, 6
PROF_CLASSES = 4


class LLPFError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("llpf status %d: %s" % (code, msg))
        self.code = code


class DegenerateWeights(LLPFError):
    pass


_lib = None


def lib():
    """Load libllpf_hip.so (fails loudly if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libllpf_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, args in SYMBOLS.items():
            if os.environ.get("LLPF_LIB") and not hasattr(L, name):
                continue             # A/B run against an older build of the engine (tools/ab): newer entry points are simply absent
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_char_p if name == "llpf_last_error" else C.c_int
        _lib = L
    return _lib


def check(code):
    if code != OK:
        msg = lib().llpf_last_error().decode("utf-8", "replace")
        if code == ERR_DEGENERATE:
            raise DegenerateWeights(code, msg)
        raise LLPFError(code, msg)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _simulate(fn, h, F, nx, nu, ny, M, T, U, u_per_trajectory, t_index0, seed, step0, flags, states, measurements):
    """llpf_simulate / llpf_bank_simulate: returns X [F, T, M, nx] (or None), Y [F, T, M, ny] (or None)"""
    M, T = int(M), int(T)
    if nu > 0:
        U = f64(U).reshape((F, M, T, nu) if u_per_trajectory else (T, nu))
    else:
        U = None
    X = np.empty((F, T, M, nx)) if states else None
    Y = np.empty((F, T, M, ny)) if measurements else None
    check(fn(h, M, T, dptr(U), 1 if u_per_trajectory else 0, float(t_index0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0) & 0xFFFFFFFF,
             int(flags), dptr(X), dptr(Y)))
    return X, Y


def device_count():
    n = C.c_int32(0)
    lib().llpf_device_count(C.byref(n))
    return n.value


class _Handle:
    """What every handle shares.  `_SYM`: the prefix of the handle's symbols, so that verb `v` is the export `_SYM_v` (llpf_<verb> for the
    filter, llpf_<kind>_<verb> for the banks); `h`: the handle, destroyed by close() or with the object."""
    _SYM = None

    def _call(self, verb, *args):
        check(getattr(self.L, "%s_%s" % (self._SYM, verb))(self.h, *args))

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._SYM + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._call("reset")

    def _scalar(self, verb, ctype):
        """a getter whose one output is a scalar of `ctype`"""
        v = ctype(0)
        self._call(verb, C.byref(v))
        return v.value

    def _profile(self, *lead):
        ms = np.zeros(PROF_CLASSES)
        n = np.zeros(PROF_CLASSES, dtype=np.int64)
        self._call("get_profile", *lead, dptr(ms), iptr(n))
        return ms, n

    def _io(self, U, Y):
        """the inputs every filter shares: U [T, nu] (None without inputs), Y [T, ny], T"""
        Y = f64(Y).reshape(-1, self.ny)
        T = Y.shape[0]
        U = f64(U).reshape(T, self.nu) if self.nu else None
        return U, Y, T


class _PfHandle(_Handle):
    """... and what the handles of particle filters share beyond that: the seed, the profile and the counters of the last run."""

    def seed(self, s):
        self._call("seed", int(s) & 0xFFFFFFFFFFFFFFFF)

    def set_profiling(self, on):
        self._call("set_profiling", 1 if on else 0)

    def profile(self):
        return self._profile()

    def last_run_ms(self):
        return self._scalar("last_run_ms", C.c_double)

    def resample_count(self):
        return self._scalar("resample_count", C.c_int64)


def _models_or_replicas(base_cfg, models, n_filters):
    """F, the (S.Model * F) array or None, and filter 0's model: one llpf_model per filter, or None with n_filters, where every filter uses
    base_cfg.model (Monte-Carlo replicas)"""
    if models is None:
        return int(n_filters), None, base_cfg.model
    F = len(models)
    return F, (S.Model * F)(*models), models[0]


class FilterHandle(_PfHandle):
    """RAII wrapper of an `llpf_filter*` (one filter on one device)."""
    _SYM = "llpf"

    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.h = _vp()
        check(self.L.llpf_create(C.byref(cfg), C.byref(self.h)))
        self.N = int(cfg.n_particles)
        self.nx, self.nu, self.ny = cfg.model.nx, cfg.model.nu, cfg.model.ny
        if cfg.model.model_id == S.MODEL_RB_BILINEAR:      # particles, history and means are [xn; xl] (RBParticle, reference src/rbpf.jl:24-30)
            self.nx = cfg.model.nx + cfg.model.rb.nxl

    # --- step ---
    def set_model(self, model):
        """new parameters, same model family and dimensions (the reference's filter_from_parameters(theta, pf)): nothing is reallocated"""
        self._call("set_model", C.byref(model))

    def _u(self, u):
        if self.nu == 0:
            return None
        u = f64(u).reshape(-1)
        if u.size != self.nu:
            raise ValueError("u must have %d elements" % self.nu)
        return u

    def _y(self, y):
        if y is None:
            return None
        y = f64(y).reshape(-1)
        if y.size != self.ny:
            raise ValueError("y must have %d elements" % self.ny)
        return y

    def _step_ll(self, verb, *args):
        """a step whose last argument is the log-likelihood it returns"""
        ll = C.c_double(0)
        self._call(verb, *args, C.byref(ll))
        return ll.value

    def correct(self, u, y, t):
        u, y = self._u(u), self._y(y)
        return self._step_ll("correct", dptr(u), dptr(y), float(t))

    def predict(self, u, t):
        u = self._u(u)
        self._call("predict", dptr(u), float(t))

    def update(self, u, y, t):
        u, y = self._u(u), self._y(y)
        return self._step_ll("update", dptr(u), dptr(y), float(t))

    def _run(self, verb, U, Y, arg, ll_steps, xmean, history, xcov=False, quantiles=None):
        """llpf_run / llpf_aux_run: the outputs asked for, as the RunOutputs of the call and as the dictionary it returns; `arg`: the
        argument between T and ll_total (t_index0, or the mode)"""
        U, Y, T = self._io(U, Y)
        outs = S.RunOutputs()
        res = {}
        if quantiles is not None:
            qp = np.ascontiguousarray(np.atleast_1d(quantiles), dtype=np.float64)
            res["xquant"] = np.zeros((T, self.nx, qp.size))
            outs.xquant, outs.quant_p, outs.nq = dptr(res["xquant"]), dptr(qp), int(qp.size)
        if xcov:
            res["xcov"] = np.zeros((T, self.nx, self.nx))
            outs.xcov = dptr(res["xcov"])
        if ll_steps:
            res["ll_steps"] = np.zeros(T)
            outs.ll_steps = dptr(res["ll_steps"])
        if xmean:
            res["xmean"] = np.zeros((T, self.nx))
            outs.xmean = dptr(res["xmean"])
        if history:
            res["x"] = np.zeros((T, self.N, self.nx))
            res["w"] = np.zeros((T, self.N))
            res["we"] = np.zeros((T, self.N))
            outs.x_hist, outs.w_hist, outs.we_hist = dptr(res["x"]), dptr(res["w"]), dptr(res["we"])
        ll = C.c_double(0)
        self._call(verb, dptr(U), dptr(Y), T, arg, C.byref(ll), C.byref(outs))
        res["ll"] = ll.value
        return res

    def run(self, U, Y, t_index0=0.0, ll_steps=False, xmean=False, history=False, xcov=False, quantiles=None):
        """quantiles: probabilities q -> res["xquant"] [T, nx, len(q)], weighted_quantile of every timestep's state on the device"""
        return self._run("run", U, Y, float(t_index0), ll_steps, xmean, history, xcov, quantiles)

    def simulate(self, M, T, U=None, u_per_trajectory=False, t_index0=0.0, seed=0, step0=0, flags=SIM_DYNAMICS_NOISE | SIM_MEASUREMENT_NOISE,
                 states=True, measurements=True):
        """llpf_simulate: M trajectories of T steps of this filter's model on the device.  U [T, nu] shared, or [M, T, nu] with
        u_per_trajectory; returns X [T, M, nx] (or None), Y [T, M, ny] (or None).  The handle is not changed."""
        X, Y = _simulate(self.L.llpf_simulate, self.h, 1, self.nx, self.nu, self.ny, M, T, U, u_per_trajectory, t_index0, seed, step0, flags,
                         states, measurements)
        return (None if X is None else X[0]), (None if Y is None else Y[0])

    def _get(self, verb, a):
        """an accessor that fills the array `a` (float64, or int64)"""
        self._call(verb, iptr(a) if a.dtype == np.int64 else dptr(a))
        return a

    def weighted_cov(self):
        """weighted_cov of the current particles under the current weights (reference src/filtering.jl:571-581), on the device"""
        return self._get("weighted_cov", np.zeros((self.nx, self.nx)))

    def weighted_quantile(self, q):
        """weighted_quantile of the current particles under the current weights (reference src/filtering.jl:583-595), on the device.
        The raw handle returns the C ABI's layout, [len(q), nx]; the mirror of the reference's function (api.weighted_quantile) transposes it
        to the reference's [state][q] nesting."""
        q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
        out = np.empty((q.size, self.nx))
        self._call("weighted_quantile", dptr(q), q.size, dptr(out))
        return out

    def rb_covariance(self):
        """x[1].R of an RBPF: the covariance of the linear substate shared by all particles."""
        nl = self.nx - self.cfg.model.nxn
        return self._get("rb_get_covariance", np.zeros((nl, nl)))

    def rb_linear_state(self):
        """per-particle Kalman state of LLPF_MODEL_RB_BILINEAR: xl [N, nxl], R [N, nxl, nxl] (fields of RBParticle)."""
        nl = self.cfg.model.rb.nxl
        xl = np.zeros((self.N, nl))
        R = np.zeros((self.N, nl, nl))
        self._call("rb_get_linear_state", dptr(xl), dptr(R))
        return xl, R

    def smooth(self, M, U, xf, wf, wef):
        """xb [T, M, nx], idx [T, M]: smooth(pf, xf, wf, wef, ll, M, u, y) — reference src/smoothing.jl:116-143."""
        xf, wf, wef = f64(xf), f64(wf), f64(wef)
        T = wf.shape[0]
        U = f64(U).reshape(T, self.nu) if self.nu else None
        xb = np.zeros((T, int(M), self.nx))
        idx = np.zeros((T, int(M)), dtype=np.int64)
        self._call("smooth", int(M), dptr(U), T, dptr(xf), dptr(wf), dptr(wef), dptr(xb), iptr(idx))
        return xb, idx

    # --- AuxiliaryParticleFilter verbs (reference src/filtering.jl:170-217) ---
    def aux_correct(self):
        return self._scalar("aux_correct", C.c_double)

    def aux_predict(self, u, y1, t):
        u, y1 = self._u(u), self._y(y1)
        self._call("aux_predict", dptr(u), dptr(y1), float(t))

    def aux_update(self, u, y1, t):
        u, y1 = self._u(u), self._y(y1)
        return self._step_ll("aux_update", dptr(u), dptr(y1), float(t))

    def run_aux(self, U, Y, mode=0, ll_steps=False, xmean=False, history=False):
        """mode 0: forward_trajectory loop, mode 1: loglik loop of the AuxiliaryParticleFilter (after reset)."""
        return self._run("aux_run", U, Y, int(mode), ll_steps, xmean, history)

    # --- accessors ---
    def index(self):
        return self._scalar("index", C.c_int64)

    def set_index(self, t):
        self._call("set_index", int(t))

    def particles(self):
        return self._get("get_particles", np.empty((self.N, self.nx)))

    def weights(self):
        return self._get("get_weights", np.empty(self.N))

    def expweights(self):
        return self._get("get_expweights", np.empty(self.N))

    def ancestors(self):
        return self._get("get_ancestors", np.empty(self.N, dtype=np.int64))

    def bins(self):
        return self._get("get_bins", np.empty(self.N))

    def set_particles(self, x):
        x = f64(x).reshape(self.N, self.nx)
        self._call("set_particles", dptr(x))

    def set_weights(self, w):
        w = f64(w).reshape(self.N)
        self._call("set_weights", dptr(w))

    def ess(self):
        return self._scalar("effective_particles", C.c_double)

    def shouldresample(self):
        return bool(self._scalar("shouldresample", C.c_int32))

    def last_resampled(self):
        return bool(self._scalar("last_resampled", C.c_int32))

    def maxw(self):
        return self._scalar("maxw", C.c_double)

    def weighted_mean(self):
        return self._get("weighted_mean", np.empty(self.nx))

    def last_run_stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._call("last_run_stats", C.byref(a), C.byref(b), C.byref(c))
        return {"fused_launches": a.value, "source_side_timesteps": b.value, "survivor_fraction": c.value}

    def last_run_form(self):
        a, b = C.c_int32(0), C.c_int64(0)
        self._call("last_run_form", C.byref(a), C.byref(b))
        return {"weights_not_stored": bool(a.value & 1), "ancestors_not_stored": bool(a.value & 2), "lean": bool(a.value & 4), "no_maximum": bool(a.value & 8), "exact_redos": b.value}


KALMAN_OUTPUTS = ("ll_steps", "x", "xt", "R", "Rt", "e")
KALMAN_SMOOTH_OUTPUTS = ("xT", "RT")


class _KfBankHandle(_Handle):
    """What the handles of the one-thread-per-filter Kalman banks share.  `times`: the arguments the bank's run and smooth take between
    per_filter and ll_total (none, or t_index0)."""

    def _open(self, models):
        self.L = lib()
        self.h = _vp()
        self.F = len(models)
        m0 = models[0]
        self.nx, self.nu, self.ny = m0.nx, m0.nu, m0.ny
        return (S.Model * self.F)(*models)

    def _inputs(self, U, Y, u_per_filter, y_per_filter):
        F, nu, ny = self.F, self.nu, self.ny
        Y = f64(Y)
        T = Y.shape[1] if y_per_filter else Y.reshape(-1, ny).shape[0]
        Y = Y.reshape((F, T, ny) if y_per_filter else (T, ny))
        if nu > 0:
            U = f64(U).reshape((F, T, nu) if u_per_filter else (T, nu))
        else:
            U, u_per_filter = None, False
        return U, Y, T, u_per_filter

    def _forward_outputs(self, T, outputs, struct=S.KalmanOutputs, more=None):
        """`struct`: the outputs' struct of the bank's run; `more`: the shapes of its members next to ll_steps, x, xt, R and Rt"""
        F, nx = self.F, self.nx
        shapes = {"ll_steps": (T, F), "x": (T, F, nx), "xt": (T, F, nx), "R": (T, F, nx, nx), "Rt": (T, F, nx, nx)}
        shapes.update({"e": (T, F, self.ny)} if more is None else more)
        res = {k: np.empty(shapes[k]) for k in outputs}
        out = None
        if res:
            out = struct()
            out.struct_size = C.sizeof(struct)
            for k, a in res.items():
                setattr(out, k, dptr(a))
        return res, out

    def _run(self, U, Y, u_per_filter, y_per_filter, outputs, *times):
        U, Y, T, u_per_filter = self._inputs(U, Y, u_per_filter, y_per_filter)
        res, out = self._forward_outputs(T, outputs)
        ll = np.empty(self.F)
        self._call("run", dptr(U), dptr(Y), T, (1 if u_per_filter else 0) | (2 if y_per_filter else 0), *times, dptr(ll),
                   None if out is None else C.byref(out))
        res["ll"] = ll
        return res

    def _smooth(self, U, Y, u_per_filter, y_per_filter, outputs, forward, *times):
        F, nx = self.F, self.nx
        U, Y, T, u_per_filter = self._inputs(U, Y, u_per_filter, y_per_filter)
        res, fwd = self._forward_outputs(T, forward)
        shapes = {"xT": (T, F, nx), "RT": (T, F, nx, nx)}
        sm = {k: np.empty(shapes[k]) for k in outputs}
        out = S.KalmanSmoothOutputs()
        out.struct_size = C.sizeof(S.KalmanSmoothOutputs)
        for k, a in sm.items():
            setattr(out, k, dptr(a))
        ll = np.empty(F)
        self._call("smooth", dptr(U), dptr(Y), T, (1 if u_per_filter else 0) | (2 if y_per_filter else 0), *times, dptr(ll),
                   None if fwd is None else C.byref(fwd), C.byref(out))
        res.update(sm)
        res["ll"] = ll
        return res

    def get_state(self):
        x = np.empty((self.F, self.nx))
        R = np.empty((self.F, self.nx, self.nx))
        self._call("get_state", dptr(x), dptr(R))
        return x, R

    def set_state(self, x, R):
        x = f64(x).reshape(self.F, self.nx)
        R = f64(R).reshape(self.F, self.nx, self.nx)
        self._call("set_state", dptr(x), dptr(R))


class _KfMatrixBankHandle(_KfBankHandle):
    """What the handles of the banks with constant matrices share: the models and D [F, ny, nu] or None."""

    def __init__(self, device, models, D=None):
        arr = self._open(models)
        D = None if D is None else f64(D).reshape(self.F, self.ny, self.nu)
        check(getattr(self.L, self._SYM + "_create")(int(device), arr, dptr(D), self.F, C.byref(self.h)))

    def set_models(self, models, D=None):
        arr = (S.Model * self.F)(*models)
        D = None if D is None else f64(D).reshape(self.F, self.ny, self.nu)
        self._call("set_models", arr, dptr(D))


class KalmanBankHandle(_KfMatrixBankHandle):
    """RAII wrapper of an `llpf_kalman_bank*` (independent Kalman filters with constant matrices on one device)."""
    _SYM = "llpf_kalman_bank"

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=()):
        """T steps of every filter: U [T, nu] or [F, T, nu] (u_per_filter), Y [T, ny] or [F, T, ny] (y_per_filter).  Returns
        {"ll": [F], name: array} for every name of `outputs` (KALMAN_OUTPUTS), time-major: ll_steps [T, F], x / xt [T, F, nx],
        R / Rt [T, F, nx, nx], e [T, F, ny]."""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs)

    def smooth(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=KALMAN_SMOOTH_OUTPUTS, forward=()):
        """the forward pass of run() and the RTS smoother's backward pass (llpf_kalman_bank_smooth).  Returns {"ll": [F]} with xT [T, F, nx]
        and RT [T, F, nx, nx] for the names in `outputs` (KALMAN_SMOOTH_OUTPUTS) and the forward outputs named in `forward`
        (KALMAN_OUTPUTS); the state afterwards is the one run() leaves."""
        return self._smooth(U, Y, u_per_filter, y_per_filter, outputs, forward)


class SqkfBankHandle(_KfMatrixBankHandle):
    """RAII wrapper of an `llpf_sqkf_bank*` (independent square-root Kalman filters with constant matrices on one device): the models,
    D, inputs and outputs of KalmanBankHandle; the state is x and a lower-triangular factor L of the covariance, R = L L'."""
    _SYM = "llpf_sqkf_bank"

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=()):
        """T steps of every filter; inputs and the returned dictionary as KalmanBankHandle.run (R and Rt are L L')"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs)

    def get_state(self, factor=False):
        """(x [F, nx], R [F, nx, nx]), R = L L'; with factor: (x, R, L), L [F, nx, nx] the lower-triangular factor itself"""
        x = np.empty((self.F, self.nx))
        R = np.empty((self.F, self.nx, self.nx))
        L = np.empty((self.F, self.nx, self.nx)) if factor else None
        self._call("get_state", dptr(x), dptr(R), dptr(L))
        return (x, R, L) if factor else (x, R)

    def set_state(self, x, R=None, L=None):
        """x and exactly one of R (a positive definite covariance, factored) and L (a factor, whose lower triangle is taken as it is:
        get_state(factor=True) -> set_state(x, L=L) keeps every bit)"""
        x = f64(x).reshape(self.F, self.nx)
        R = None if R is None else f64(R).reshape(self.F, self.nx, self.nx)
        L = None if L is None else f64(L).reshape(self.F, self.nx, self.nx)
        self._call("set_state", dptr(x), dptr(R), dptr(L))


IMM_OUTPUTS = ("ll_steps", "x", "xt", "R", "Rt", "mu", "ll_modes")
IMM_INTERACT = 1
IMM_EXTENDED = 2


class IMMBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_imm_bank*` (independent IMM filters of M modes each on one device, one lane per mode).
    `models`: [F][M] descriptors (a list of F lists of M), D [F, M, ny, nu] or None, P [F, M, M], mu0 [F, M].  extended: the modes are
    first-order extended Kalman filters of one model type (LLPF_IMM_EXTENDED; implied by a model other than the linear-Gaussian one), D None.
    unscented: the modes are unscented Kalman filters of one model type (llpf_imm_bank_create_unscented), D None, `weights` =
    (gamma, wm0, wc0, wi) the one set of the bank."""
    _SYM = "llpf_imm_bank"

    def __init__(self, device, models, D, P, mu0, interact=True, extended=False, unscented=False, weights=None):
        self.M = len(models[0]) if len(models) else 0
        if any(len(row) != self.M for row in models):
            raise ValueError("every filter of an IMM bank has the same number of modes")
        if unscented and (extended or D is not None or weights is None):
            raise ValueError("an unscented IMM bank is not extended, has no D and needs weights")
        if weights is not None and not unscented:
            raise ValueError("only an unscented IMM bank has weights")
        arr = self._pack(models, first=True)
        D, P, mu0 = self._tables(D, P, mu0)
        if unscented:
            w = ukf_weights(weights)
            check(self.L.llpf_imm_bank_create_unscented(int(device), arr, dptr(P), dptr(mu0), self.F, self.M, IMM_INTERACT if interact else 0,
                                                        C.byref(w), C.byref(self.h)))
            return
        check(self.L.llpf_imm_bank_create(int(device), arr, dptr(D), dptr(P), dptr(mu0), self.F, self.M,
                                          (IMM_INTERACT if interact else 0) | (IMM_EXTENDED if extended else 0), C.byref(self.h)))

    def _pack(self, models, first=False):
        flat = [m for row in models for m in row]
        if first:
            self._open(flat if flat else [S.Model()])
            self.F = len(models)
        return (S.Model * max(len(flat), 1))(*flat)

    def _tables(self, D, P, mu0):
        F, M = self.F, self.M
        D = None if D is None else f64(D).reshape(F, M, self.ny, self.nu)
        return D, f64(P).reshape(F, M, M), f64(mu0).reshape(F, M)

    def set_models(self, models, D, P, mu0):
        arr = self._pack(models)
        D, P, mu0 = self._tables(D, P, mu0)
        self._call("set_models", arr, dptr(D), dptr(P), dptr(mu0))

    def set_weights(self, weights):
        """new (gamma, wm0, wc0, wi) for a bank of unscented modes"""
        w = ukf_weights(weights)
        self._call("set_weights", C.byref(w))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts (a bank of Kalman modes ignores the time); inputs as
        KalmanBankHandle.run.  Returns {"ll": [F], name: array} for every name of `outputs` (IMM_OUTPUTS), time-major: ll_steps [T, F],
        x / xt [T, F, nx], R / Rt [T, F, nx, nx] (the combined estimate), mu / ll_modes [T, F, M]."""
        U, Y, T, u_per_filter = self._inputs(U, Y, u_per_filter, y_per_filter)
        res, out = self._forward_outputs(T, outputs, S.ImmOutputs, {"mu": (T, self.F, self.M), "ll_modes": (T, self.F, self.M)})
        ll = np.empty(self.F)
        self._call("run_at", dptr(U), dptr(Y), T, (1 if u_per_filter else 0) | (2 if y_per_filter else 0), float(t_index0), dptr(ll),
                   None if out is None else C.byref(out))
        res["ll"] = ll
        return res

    def get_state(self):
        """the combined (x [F, nx], R [F, nx, nx])"""
        return self.get_modes()[:2]

    def get_modes(self):
        """(x [F, nx], R [F, nx, nx], mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx])"""
        F, M, nx = self.F, self.M, self.nx
        x, R, mu = np.empty((F, nx)), np.empty((F, nx, nx)), np.empty((F, M))
        xm, Rm = np.empty((F, M, nx)), np.empty((F, M, nx, nx))
        self._call("get_state", dptr(x), dptr(R), dptr(mu), dptr(xm), dptr(Rm))
        return x, R, mu, xm, Rm

    def set_state(self, mu, x_modes, R_modes):
        F, M, nx = self.F, self.M, self.nx
        mu, xm, Rm = f64(mu).reshape(F, M), f64(x_modes).reshape(F, M, nx), f64(R_modes).reshape(F, M, nx, nx)
        self._call("set_state", dptr(mu), dptr(xm), dptr(Rm))


def ukf_weights(w):
    """(gamma, wm0, wc0, wi) as an llpf_ukf_weights"""
    gamma, wm0, wc0, wi = (float(v) for v in w)
    return S.UkfWeights(C.sizeof(S.UkfWeights), 0, gamma, wm0, wc0, wi)


class UkfBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_ukf_bank*` (independent unscented Kalman filters on one device); `weights` = (gamma, wm0, wc0, wi)."""
    _SYM = "llpf_ukf_bank"

    def __init__(self, device, models, weights):
        arr = self._open(models)
        w = ukf_weights(weights)
        check(self.L.llpf_ukf_bank_create(int(device), arr, self.F, C.byref(w), C.byref(self.h)))

    def set_models(self, models):
        self._call("set_models", (S.Model * self.F)(*models))

    def set_weights(self, weights):
        w = ukf_weights(weights)
        self._call("set_weights", C.byref(w))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.run"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs, float(t_index0))

    def smooth(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=KALMAN_SMOOTH_OUTPUTS, forward=(), t_index0=0.0):
        """the forward pass of run() and the unscented RTS smoother's backward pass (llpf_ukf_bank_smooth), step t at time
        (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.smooth"""
        return self._smooth(U, Y, u_per_filter, y_per_filter, outputs, forward, float(t_index0))


class AukfBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_aukf_bank*` (independent unscented Kalman filters with augmented process noise on one device);
    `weights` = the pair (measurement set, dynamics set), each (gamma, wm0, wc0, wi): the first for L = nx, the second for L = 2 nx."""
    _SYM = "llpf_aukf_bank"

    def __init__(self, device, models, weights):
        arr = self._open(models)
        wm, wd = (ukf_weights(w) for w in weights)
        check(self.L.llpf_aukf_bank_create(int(device), arr, self.F, C.byref(wm), C.byref(wd), C.byref(self.h)))

    def set_models(self, models):
        self._call("set_models", (S.Model * self.F)(*models))

    def set_weights(self, weights):
        wm, wd = (ukf_weights(w) for w in weights)
        self._call("set_weights", C.byref(wm), C.byref(wd))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.run"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs, float(t_index0))


class EkfBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_ekf_bank*` (independent extended Kalman filters on one device)."""
    _SYM = "llpf_ekf_bank"

    def __init__(self, device, models):
        arr = self._open(models)
        check(self.L.llpf_ekf_bank_create(int(device), arr, self.F, C.byref(self.h)))

    def set_models(self, models):
        self._call("set_models", (S.Model * self.F)(*models))

    def set_iterations(self, maxiters, epsilon):
        """the iterated filter for every later run: at most `maxiters` linearisations of a step's measurement, stopped once no state moved
        by more than `epsilon`; (1, 0.0) is the plain filter (llpf_ekf_bank_set_iterations)"""
        self._call("set_iterations", int(maxiters), float(epsilon))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.run"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs, float(t_index0))


class SqekfBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_sqekf_bank*` (independent square-root extended Kalman filters on one device): the models, inputs and
    outputs of EkfBankHandle; the state is x and a lower-triangular factor L of the covariance, R = L L', as SqkfBankHandle's."""
    _SYM = "llpf_sqekf_bank"

    def __init__(self, device, models):
        arr = self._open(models)
        check(self.L.llpf_sqekf_bank_create(int(device), arr, self.F, C.byref(self.h)))

    def set_models(self, models):
        self._call("set_models", (S.Model * self.F)(*models))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.run (R and
        Rt are L L')"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs, float(t_index0))

    get_state = SqkfBankHandle.get_state
    set_state = SqkfBankHandle.set_state


class EnkfBankHandle(_KfBankHandle):
    """RAII wrapper of an `llpf_enkf_bank*` (independent ensemble Kalman filters of `n_members` members on one device; filter f's key is
    seed + f)."""
    _SYM = "llpf_enkf_bank"

    def __init__(self, device, models, n_members, seed=0):
        arr = self._open(models)
        self.N = int(n_members)
        check(self.L.llpf_enkf_bank_create(int(device), arr, self.F, self.N, int(seed), C.byref(self.h)))

    def set_models(self, models):
        self._call("set_models", (S.Model * self.F)(*models))

    def set_inflation(self, rho):
        """the inflation of every later predict!: x_i = mean + rho (x_i - mean); finite and >= 1"""
        self._call("set_inflation", float(rho))

    def seed(self, seed):
        """zeroes the counters of the generator and draws the first ensemble of `seed`: the bank a create with that seed gives"""
        self._call("seed", int(seed))

    def run(self, U, Y, u_per_filter=False, y_per_filter=False, outputs=(), t_index0=0.0):
        """T steps of every filter, step t at time (t_index0 + t) Ts; inputs and the returned dictionary as KalmanBankHandle.run"""
        return self._run(U, Y, u_per_filter, y_per_filter, outputs, float(t_index0))

    def _u(self, u, u_per_filter):
        if self.nu == 0:
            return None, False
        return f64(u).reshape((self.F, self.nu) if u_per_filter else (self.nu,)), u_per_filter

    def correct(self, u, y, u_per_filter=False, y_per_filter=False, t_index=0.0):
        """correct!(u, y) of every filter at time t_index Ts: (ll [F], e [F, ny]); u [nu] or [F, nu], y [ny] or [F, ny]"""
        u, u_per_filter = self._u(u, u_per_filter)
        y = f64(y).reshape((self.F, self.ny) if y_per_filter else (self.ny,))
        ll, e = np.empty(self.F), np.empty((self.F, self.ny))
        self._call("correct", dptr(u), dptr(y), (1 if u_per_filter else 0) | (2 if y_per_filter else 0), float(t_index), dptr(ll), dptr(e))
        return ll, e

    def predict(self, u, u_per_filter=False, t_index=0.0):
        """predict!(u) of every filter at time t_index Ts"""
        u, u_per_filter = self._u(u, u_per_filter)
        self._call("predict", dptr(u), 1 if u_per_filter else 0, float(t_index))

    def get_members(self):
        """the members of every filter, [F, N, nx]"""
        X = np.empty((self.F, self.N, self.nx))
        self._call("get_members", dptr(X))
        return X

    def set_members(self, X):
        X = f64(X).reshape(self.F, self.N, self.nx)
        self._call("set_members", dptr(X))

    def set_state(self, x, R):
        raise TypeError("an ensemble Kalman filter's state is its members: use set_members")


class BankHandle(_PfHandle):
    """RAII wrapper of an `llpf_bank*` (many independent filters on one device)."""
    _SYM = "llpf_bank"

    def __init__(self, base_cfg, models=None, n_filters=None):
        """models: one llpf_model per filter, or None with n_filters: every filter uses base_cfg.model (Monte-Carlo replicas)."""
        self.L = lib()
        self.cfg = base_cfg
        self.h = _vp()
        self.F, self._models, m0 = _models_or_replicas(base_cfg, models, n_filters)
        check(self.L.llpf_bank_create(C.byref(base_cfg), self._models, self.F, C.byref(self.h)))
        self.N = int(base_cfg.n_particles)
        self.nx, self.nu, self.ny = m0.nx, m0.nu, m0.ny

    def set_models(self, models):
        """new parameters for every filter of the bank (len(models) == n_filters), same model family and dimensions"""
        if len(models) != self.F:
            raise ValueError("set_models: %d models for a bank of %d filters" % (len(models), self.F))
        arr = (S.Model * self.F)(*models)
        self._call("set_models", arr)
        self._models = arr

    def run(self, U, Y, t_index0=0.0, ll_steps=False):
        U, Y, T = self._io(U, Y)
        ll = np.zeros(self.F)
        lls = np.zeros((T, self.F)) if ll_steps else None
        self._call("run", dptr(U), dptr(Y), T, float(t_index0), dptr(ll), dptr(lls))
        return {"ll": ll, "ll_steps": lls}

    def run_multi(self, U, Y, t_index0=0.0, ll_steps=False, xmean=False):
        """every filter runs on inputs of its own: U [F, T, nu], Y [F, T, ny]; xmean -> [T, F, nx] weighted means after correct!"""
        Y = f64(Y).reshape(self.F, -1, self.ny)
        T = Y.shape[1]
        U = f64(U).reshape(self.F, T, self.nu) if self.nu else None
        ll = np.zeros(self.F)
        lls = np.zeros((T, self.F)) if ll_steps else None
        xm = np.zeros((T, self.F, self.nx)) if xmean else None
        self._call("run_multi", dptr(U), dptr(Y), T, float(t_index0), dptr(ll), dptr(lls), dptr(xm))
        return {"ll": ll, "ll_steps": lls, "xmean": xm}

    def run_aux(self, U, Y, mode=1, ll_steps=False):
        U, Y, T = self._io(U, Y)
        ll = np.zeros(self.F)
        lls = np.zeros((T, self.F)) if ll_steps else None
        self._call("aux_run", dptr(U), dptr(Y), T, int(mode), dptr(ll), dptr(lls))
        return {"ll": ll, "ll_steps": lls}

    def simulate(self, M, T, U=None, u_per_trajectory=False, t_index0=0.0, seed=0, step0=0, flags=SIM_DYNAMICS_NOISE | SIM_MEASUREMENT_NOISE,
                 states=True, measurements=True):
        """llpf_bank_simulate: M trajectories of every filter's model, filter k with key seed + k.  U [T, nu] shared, or [F, M, T, nu] with
        u_per_trajectory; returns X [F, T, M, nx] (or None), Y [F, T, M, ny] (or None)."""
        return _simulate(self.L.llpf_bank_simulate, self.h, self.F, self.nx, self.nu, self.ny, M, T, U, u_per_trajectory, t_index0, seed, step0,
                         flags, states, measurements)


MBANK_ID_BYTES = 128
MBANK_COLL = {0: "none", 1: "rccl", 2: "host", 3: "external"}


def mbank_unique_id():
    """ncclGetUniqueId through the C ABI (rank 0 of a one-process-per-GPU job; the host distributes the bytes)."""
    buf = (C.c_uint8 * MBANK_ID_BYTES)()
    check(lib().llpf_mbank_unique_id(buf))
    return bytes(buf)


class MBankHandle(_PfHandle):
    """RAII wrapper of an `llpf_mbank*`: a sweep of independent filters sharded over GPUs, filter k on shard k mod n_shards;
    the exchange of the log-likelihood vector (RCCL) happens inside run().

    devices=[...]             : this process drives all listed GPUs (llpf_mbank_create)
    rank=, world=, unique_id= : one process per GPU (llpf_mbank_create_rank); unique_id None with world > 1 leaves the
                                exchange to the caller (run() then returns this rank's slots, zeros elsewhere)"""
    _SYM = "llpf_mbank"

    def __init__(self, base_cfg, models=None, n_filters=None, devices=None, rank=None, world=None, unique_id=None):
        self.L = lib()
        self.cfg = base_cfg
        self.h = _vp()
        self.F, arr, m0 = _models_or_replicas(base_cfg, models, n_filters)
        self._models = arr
        if rank is None:
            devs = list(devices if devices is not None else [base_cfg.device])
            darr = (C.c_int32 * len(devs))(*devs)
            check(self.L.llpf_mbank_create(C.byref(base_cfg), arr, self.F, darr, len(devs), C.byref(self.h)))
        else:
            idp = None
            if unique_id is not None:
                if len(unique_id) != MBANK_ID_BYTES:
                    raise ValueError("unique_id must have %d bytes" % MBANK_ID_BYTES)
                idp = (C.c_uint8 * MBANK_ID_BYTES)(*unique_id)
            check(self.L.llpf_mbank_create_rank(C.byref(base_cfg), arr, self.F, int(rank), int(world), idp, C.byref(self.h)))
        self.N = int(base_cfg.n_particles)
        self.nx, self.nu, self.ny = m0.nx, m0.nu, m0.ny

    def set_models(self, models):
        """new parameters for every filter of the sweep (all n_filters descriptors, on every rank)"""
        if len(models) != self.F:
            raise ValueError("set_models: %d models for a sweep of %d filters" % (len(models), self.F))
        arr = (S.Model * self.F)(*models)
        self._call("set_models", arr)
        self._models = arr

    def _sweep(self, verb, U, Y, arg):
        U, Y, T = self._io(U, Y)
        ll = np.zeros(self.F)
        tot = C.c_double(0)
        self._call(verb, dptr(U), dptr(Y), T, arg, dptr(ll), C.byref(tot))
        return {"ll": ll, "ll_sum": tot.value}

    def run(self, U, Y, t_index0=0.0):
        return self._sweep("run", U, Y, float(t_index0))

    def run_aux(self, U, Y, mode=1):
        return self._sweep("aux_run", U, Y, int(mode))

    def info(self):
        i = S.MBankInfo()
        self._call("info", C.byref(i))
        d = {k: getattr(i, k) for k, _ in S.MBankInfo._fields_}
        d["collective"] = MBANK_COLL.get(d["collective"], d["collective"])
        devs = (C.c_int32 * max(1, i.n_local_shards))()
        self._call("local_devices", devs)
        d["local_devices"] = list(devs)[: i.n_local_shards]
        return d

    def last_run_ms(self):
        return self.info()["last_run_ms"]

    def resample_count(self):
        return self.info()["resample_count"]

    def profile(self, local_shard=0):
        return self._profile(int(local_shard))


def mbank_partition(n_filters, shard, n_shards):
    """llpf_mbank_partition: global indices of the filters shard `shard` of `n_shards` owns (pure host code)"""
    n = C.c_int32(0)
    check(lib().llpf_mbank_partition(int(n_filters), int(shard), int(n_shards), None, C.byref(n)))
    a = (C.c_int32 * max(1, n.value))()
    check(lib().llpf_mbank_partition(int(n_filters), int(shard), int(n_shards), a, C.byref(n)))
    return [int(a[i]) for i in range(n.value)]


def model_compile(device_src, nx, ny):
    """llpf_model_compile: JIT a user model (HIP source defining `struct UserModel`, include/llpf.h); returns the model id
    to put into llpf_model.model_id"""
    mid = C.c_int32(-1)
    check(lib().llpf_model_compile(device_src.encode("utf-8"), int(nx), int(ny), C.byref(mid)))
    return mid.value


TRAIT_LOGLIK, TRAIT_LOGLIK_BOUND, TRAIT_NOISE, TRAIT_INITIAL = 1, 2, 4, 8
TRAIT_DYNAMICS_JAC, TRAIT_MEASUREMENT_JAC = 16, 32
TRAIT_DYNAMICS_W = 64


def model_traits(model_id):
    """llpf_model_traits: which optional members (loglik, loglik_bound, noise, initial, dynamics_jac, measurement_jac) a compiled model has, as TRAIT_* bits"""
    t = C.c_int32(0)
    check(lib().llpf_model_traits(int(model_id), C.byref(t)))
    return t.value


# array primitives -----------------------------------------------------------------------------------
def logsumexp(w, device=0):
    """ll, w_normalised, we = logsumexp!(w, we)  (reference src/utils.jl:18-27), computed on the GPU."""
    w = f64(w).copy()
    we = np.empty_like(w)
    ll = C.c_double(0)
    check(lib().llpf_logsumexp(device, dptr(w), dptr(we), w.size, C.byref(ll)))
    return ll.value, w, we


def resample(strategy, we, U, m=None, j0=None, device=0):
    """j = resample(strategy, we, M) (reference src/resample.jl:12-61), 0-based, computed on the GPU."""
    we = f64(we)
    n = we.size
    m = n if m is None else int(m)
    j = np.zeros(m, dtype=np.int64) if j0 is None else np.ascontiguousarray(j0, dtype=np.int64).copy()
    U = f64(np.atleast_1d(U))
    need = 1 if strategy == S.RESAMPLE_SYSTEMATIC else m
    if U.size < need or j.size < m:
        raise ValueError("resample: %d uniform(s) and %d ancestor slots are needed" % (need, m))
    check(lib().llpf_resample(device, strategy, dptr(we), n, m, dptr(U), iptr(j)))
    return j


def resample_uniforms(strategy, m, seed, step):
    u = np.zeros(1 if strategy == S.RESAMPLE_SYSTEMATIC else m)
    check(lib().llpf_resample_uniforms(strategy, m, int(seed) & 0xFFFFFFFFFFFFFFFF, step, dptr(u)))
    return u


def selftest_math(which, x, device=0):
    x = f64(x)
    out = np.empty_like(x)
    check(lib().llpf_selftest_math(device, which, dptr(x), dptr(out), x.size))
    return out


def selftest_normals(seed, step, stream, nd, n, device=0):
    out = np.empty((n, nd))
    check(lib().llpf_selftest_normals(device, int(seed), step, stream, nd, dptr(out), n))
    return out
