"""Host-side mirror of the reference's particle-filter API for the hot path.

Names follow LowLevelParticleFilters.jl (exports: reference src/LowLevelParticleFilters.jl:3-16) with the
trailing `!` dropped (`reset!` -> `reset`, `predict!` -> `predict`, `correct!` -> `correct`,
`update!` -> `update`, `logsumexp!` -> `logsumexp`).  Every verb is a thin call into the C ABI
(include/llpf.h); nothing here computes particle data on the host, and there is no fallback when
the GPU library is missing.

A closure cannot run on the GPU, so the `dynamics` / `measurement` /
`measurement_likelihood` arguments are *model descriptors*:

    LinearDynamics(A, B), LinearMeasurement(C)        x+ = A x + B u,  y = C x
    QuadTankDynamics(...), QuadTankMeasurement()      reference examples/example_quadtank.jl:8-35
    GaussianLikelihood(measurement, dg)               logpdf(dg, y - g(x)) for AdvancedParticleFilter
    UserDynamics(src, ...) + UserMeasurement / ...    HIP source of a model of one's own (llpf_model_compile)

— or, since round 6, ordinary Python callables with the reference's signatures (`dynamics(x, u, p, t)`, `measurement(x, u, p, t)`,
`measurement_likelihood(x, u, y, p, t)`; pass `nu=` / `ny=`): straight-line functions are traced once on tracer numbers and emitted as
the device snippet (tracing.py), operation for operation.
"""
import ctypes as C

import numpy as np

from . import _capi
from . import _structs as S

__all__ = [
    "StateAffineCoupling",
    "MvNormal", "ResampleSystematic", "ResampleStratified",
    "LinearDynamics", "LinearMeasurement", "QuadTankDynamics", "QuadTankMeasurement", "GaussianLikelihood",
    "ResampleResidual", "weighted_cov", "weighted_quantile", "log_likelihood_fun", "metropolis", "metropolis_bank", "naive_sampler", "mode_trajectory", "KalmanFilter", "KalmanFilterBank", "SqKalmanFilter", "SqKalmanFilterBank", "KalmanFilteringSolution", "KalmanSmoothingSolution", "covariance", "UnscentedKalmanFilter", "UnscentedKalmanFilterBank", "AugmentedUnscentedKalmanFilter", "AugmentedUnscentedKalmanFilterBank", "ExtendedKalmanFilter", "ExtendedKalmanFilterBank", "IteratedExtendedKalmanFilter", "IteratedExtendedKalmanFilterBank", "SqExtendedKalmanFilter", "SqExtendedKalmanFilterBank", "EnsembleKalmanFilter", "EnsembleKalmanFilterBank", "IMM", "IMMBank", "IMMFilteringSolution", "MerweParams", "WikiParams", "TrivialParams", "RBMeasurementModel", "RBPF", "smooth", "smoothed_mean", "smoothed_cov", "smoothed_trajs", "ParticleFilter", "AdvancedParticleFilter", "AuxiliaryParticleFilter", "FilterBank", "ParticleFilteringSolution",
    "reset", "predict", "correct", "update", "forward_trajectory", "mean_trajectory", "loglik",
    "particles", "weights", "expweights", "state", "num_particles", "index", "effective_particles",
    "shouldresample", "resample", "weighted_mean", "logsumexp", "simulate", "simulate_batch", "parameters",
    "dynamics", "measurement", "measurement_likelihood", "dynamics_density", "measurement_density",
    "initial_density", "resample_threshold", "resampling_strategy", "UserDynamics", "UserMeasurement", "UserLikelihood", "UserNoise", "UserInitial",
]


# ---------------------------------------------------------------------------------------------------
# densities and model descriptors
# ---------------------------------------------------------------------------------------------------
class MvNormal:
    """N(mu, Sigma).  `cov`: float -> sigma^2 * I (PDMats.ScalMat), 1-D array -> diagonal (PDiagMat),
    2-D array -> full (PDMat).  Mirrors Distributions.MvNormal / SimpleMvNormal as used by the
    reference (src/utils.jl:241-270, ext/LowLevelParticleFiltersDistributionsExt.jl:16,80)."""

    def __init__(self, mu, cov=None, kind=None):
        if cov is None:            # MvNormal(Sigma): zero mean
            cov = mu
            c = np.asarray(cov, dtype=np.float64)
            if c.ndim == 0:
                raise ValueError("MvNormal(cov) needs an array covariance to infer the dimension")
            mu = np.zeros(c.shape[0])
        self._g = S.make_gaussian(mu, cov, kind)

    def __len__(self):
        return self._g.dim

    @property
    def mean(self):
        return S.gaussian_mean(self._g)

    @property
    def cov(self):
        return S.gaussian_cov_matrix(self._g)

    def rand(self, rng):
        return self.mean + np.linalg.cholesky(self.cov) @ rng.standard_normal(len(self))

    def struct(self):
        return self._g


class ResampleSystematic:      # reference src/LowLevelParticleFilters.jl:44
    code = S.RESAMPLE_SYSTEMATIC


class ResampleStratified:      # reference src/LowLevelParticleFilters.jl:45
    code = S.RESAMPLE_STRATIFIED


class ResampleResidual:        # reference src/LowLevelParticleFilters.jl:46, src/resample.jl:63-117
    code = S.RESAMPLE_RESIDUAL


class LinearDynamics:
    def __init__(self, A, B=None):
        self.A = np.atleast_2d(np.asarray(A, dtype=np.float64))
        self.B = None if B is None else np.asarray(B, dtype=np.float64).reshape(self.A.shape[0], -1)

    def __call__(self, x, u, p=None, t=0.0):
        x = np.asarray(x, dtype=np.float64)
        out = self.A @ x
        if self.B is not None and self.B.shape[1]:
            out = out + self.B @ np.asarray(u, dtype=np.float64).reshape(-1)
        return out


class LinearMeasurement:
    def __init__(self, Cm):
        self.C = np.atleast_2d(np.asarray(Cm, dtype=np.float64))

    def __call__(self, x, u=None, p=None, t=0.0):
        return self.C @ np.asarray(x, dtype=np.float64)


class QuadTankDynamics:
    """Quad-tank process discretised with rk4 (reference examples/example_quadtank.jl:8-35,
    src/utils.jl:220-237)."""

    def __init__(self, supersample=2, **consts):
        self.supersample = int(supersample)
        self.consts = dict(S.QUADTANK_DEFAULTS)
        self.consts.update(consts)

    def rhs(self, h, u, t):
        c = self.consts
        a1 = c["a1"] * (c["a1_factor"] if t > c["t_switch"] else 1.0)
        ss = lambda z: np.sqrt(max(z, 0.0) + c["eps"])
        g2 = 2.0 * c["g"]
        return np.array([
            -a1 / c["A1"] * ss(g2 * h[0]) + c["a3"] / c["A1"] * ss(g2 * h[2]) + c["gamma1"] * c["k1"] / c["A1"] * u[0],
            -c["a2"] / c["A2"] * ss(g2 * h[1]) + c["a4"] / c["A2"] * ss(g2 * h[3]) + c["gamma2"] * c["k2"] / c["A2"] * u[1],
            -c["a3"] / c["A3"] * ss(g2 * h[2]) + (1 - c["gamma2"]) * c["k2"] / c["A3"] * u[1],
            -c["a4"] / c["A4"] * ss(g2 * h[3]) + (1 - c["gamma1"]) * c["k1"] / c["A4"] * u[0]])

    def __call__(self, x, u, p=None, t=0.0, Ts=1.0):
        x = np.asarray(x, dtype=np.float64).copy()
        h = Ts / self.supersample
        for _ in range(self.supersample):
            f1 = self.rhs(x, u, t)
            f2 = self.rhs(x + h / 2 * f1, u, t + h / 2)
            f3 = self.rhs(x + h / 2 * f2, u, t + h / 2)
            f4 = self.rhs(x + h * f3, u, t + h)
            x = x + h / 6 * (f1 + 2 * f2 + 2 * f3 + f4)
            t += h
        return x


class QuadTankMeasurement:
    def __call__(self, x, u=None, p=None, t=0.0):
        return np.asarray(x, dtype=np.float64)[:2].copy()


class GaussianLikelihood:
    """measurement_likelihood(x,u,y,p,t) = logpdf(dg, y - measurement(x,u,p,t))."""

    def __init__(self, measurement, measurement_density):
        self.measurement = measurement
        self.measurement_density = measurement_density


class UserDynamics:
    """A model the engine has no built-in for: HIP device source defining `struct UserModel` — prepare / dynamics / measurement and,
    optionally, `loglik` + `loglik_bound` (a measurement likelihood of its own) — compiled for the GPU with hiprtc when the filter
    is built (include/llpf.h: llpf_model_compile).  A, B, C, qt fill the parameter block the snippet reads (m->A, ..., m->qt[16]);
    `host` (optional) is the same dynamics as a Python callable, used only by host-side simulate."""

    def __init__(self, src, nx, nu, ny, A=None, B=None, C=None, qt=(), supersample=1, host=None):
        self.src, self.nx, self.nu, self.ny = str(src), int(nx), int(nu), int(ny)
        self.A, self.B, self.C, self.qt, self.supersample, self.host = A, B, C, list(qt), int(supersample), host

    def __call__(self, x, u=None, p=None, t=0.0, noise=False):
        if self.host is None:
            raise TypeError("no host version of this device model was given")
        return self.host(x, u, p, t)


class UserMeasurement:
    """the measurement of a UserDynamics snippet (`UserModel::measurement`); `host`: the same as a Python callable, for simulate"""

    def __init__(self, host=None):
        self.host = host

    def __call__(self, x, u=None, p=None, t=0.0, noise=False):
        if self.host is None:
            raise TypeError("no host version of this device model was given")
        return self.host(x, u, p, t)


class UserLikelihood:
    """measurement_likelihood(x, u, y, p, t) of an AdvancedParticleFilter (reference src/PFtypes.jl:226-239) as the `loglik(x, y, t)`
    member of the paired UserDynamics snippet; its `loglik_bound()` member declares the upper bound the normalisation works
    against (without one every step is normalised against the true maximum: one more launch per step, ≈ 20 % slower)."""

    def __init__(self, host=None):
        self.host = host

    def __call__(self, x, u, y, p=None, t=0.0):
        if self.host is None:
            raise TypeError("no host version of this device likelihood was given")
        return self.host(x, u, y, p, t)


class UserNoise:
    """dynamics_density of a filter whose model adds its own process noise: the `noise(x, fx, xi, uu, out)` member of the paired
    UserDynamics snippet — the reference's AdvancedParticleFilter contract, dynamics(x, u, p, t, noise = true) (src/PFtypes.jl:242-259),
    or a ParticleFilter with a dynamics_density that is not Gaussian (rand!(rng, d, noise), :122-139).  `gaussian`: the MvNormal the
    auxiliary filter's add_noise! keeps using (default: standard normal).  The FFBS smoother weights with logpdf(dynamics_density, .),
    which such a model does not have: smooth(pf, ...) raises."""

    def __init__(self, gaussian=None, host=None):
        self.gaussian, self.host = gaussian, host


class UserInitial:
    """initial_density of a filter whose model draws its own initial particles: the `initial(xi, uu, out)` member of the paired
    UserDynamics snippet (x_i = rand(rng, initial_density), reference src/filtering.jl:4-14)."""

    def __init__(self, host=None):
        self.host = host


_DESCRIPTORS = ()      # filled below: the descriptor classes a constructor accepts as they are


def _is_plain_callable(f):
    return callable(f) and not isinstance(f, _DESCRIPTORS)


def _trace_callables(dyn, meas, mlik, nx, nu, ny, p, likelihood_bound=None, jacobians=False, noise_input=False):
    """The reference's constructors take closures (src/PFtypes.jl:59-63, 189-193).  Plain Python callables with the reference's signatures
    — dynamics(x, u, p, t), measurement(x, u, p, t), measurement_likelihood(x, u, y, p, t) — are traced once (tracing.py) and emitted
    as the device snippet; returns the (UserDynamics, UserMeasurement, UserLikelihood | None) descriptors that stand for them."""
    from . import tracing
    if not _is_plain_callable(meas):
        raise TypeError("a callable dynamics needs a callable measurement (both are traced into one device model)")
    if nu < 0:
        raise ValueError("pass nu= (the number of inputs) with callable dynamics: it cannot be read off a closure")
    d = tracing.traced_dynamics(dyn, nx, nu, p=p, measurement=meas, ny=ny, measurement_likelihood=mlik if _is_plain_callable(mlik) else None,
                                loglik_bound=likelihood_bound, jacobians=jacobians, noise_input=noise_input)
    return d, d.measurement_model, d.likelihood_model


def _build_model(dyn, meas, df, dg, d0, Ts, user_likelihood=False):
    if isinstance(dyn, UserDynamics):
        if not isinstance(meas, UserMeasurement):
            raise TypeError("pair UserDynamics with UserMeasurement (the snippet's own measurement)")
        m = S.Model()
        m.model_id = _capi.model_compile(dyn.src, dyn.nx, dyn.ny)
        # what the snippet defines must be what the filter was told to use: a missing member would silently fall back to the Gaussian
        # descriptor, a present one silently override it
        traits = _capi.model_traits(m.model_id)
        for what, wanted, bit, member in (("measurement likelihood", user_likelihood, _capi.TRAIT_LOGLIK, "loglik"),
                                          ("dynamics_density", isinstance(df, UserNoise), _capi.TRAIT_NOISE, "noise"),
                                          ("initial_density", isinstance(d0, UserInitial), _capi.TRAIT_INITIAL, "initial")):
            if wanted and not traits & bit:
                raise TypeError("the %s is a User* descriptor but the snippet defines no `%s` member" % (what, member))
            if not wanted and traits & bit:
                raise TypeError("the snippet defines `%s`, which would override the Gaussian %s: pass the matching User* descriptor" % (member, what))
        if isinstance(df, UserNoise):
            df = df.gaussian if df.gaussian is not None else MvNormal(np.zeros(dyn.nx), 1.0)
        if isinstance(d0, UserInitial):
            d0 = MvNormal(np.zeros(dyn.nx), 1.0)
        m.nx, m.nu, m.ny = dyn.nx, dyn.nu, dyn.ny
        for name, mat in (("A", dyn.A), ("B", dyn.B), ("C", dyn.C)):
            if mat is not None:
                for i, v in enumerate(np.asarray(mat, dtype=np.float64).reshape(-1)):
                    getattr(m, name)[i] = v
        for i, v in enumerate(dyn.qt):
            m.qt[i] = float(v)
        m.supersample, m.Ts = dyn.supersample, float(Ts)
        m.dynamics_density, m.measurement_density, m.initial_density = df.struct(), dg.struct(), d0.struct()
        return m
    if isinstance(dyn, LinearDynamics) and isinstance(meas, LinearMeasurement):
        return S.make_lg_model(dyn.A, dyn.B, meas.C, df.struct(), dg.struct(), d0.struct(), Ts)
    if isinstance(dyn, QuadTankDynamics) and isinstance(meas, QuadTankMeasurement):
        return S.make_quadtank_model(df.struct(), dg.struct(), d0.struct(), Ts, dyn.supersample, **dyn.consts)
    raise TypeError("dynamics / measurement must be model descriptors (LinearDynamics + LinearMeasurement, QuadTankDynamics + "
                    "QuadTankMeasurement, UserDynamics + UserMeasurement) or a pair of plain callables (traced: tracing.py)")


# ---------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------
class _AbstractParticleFilter:
    kind = S.PARTICLE_FILTER

    def _setup(self, N, dyn, meas, df, dg, d0, resample_threshold, resampling_strategy, rng, p, threads, Ts, nu, ny, device):
        self.dynamics = dyn
        self.measurement = meas
        self.dynamics_density = df
        self.measurement_density = dg
        self.initial_density = d0
        self.resample_threshold = float(resample_threshold)
        self.resampling_strategy = resampling_strategy
        self.rng = 0 if rng is None else int(rng)       # the Philox key (the reference stores an Xoshiro, src/PFtypes.jl:30)
        self.p = p
        self.threads = threads                          # accepted for signature parity; the GPU is always parallel
        self.Ts = float(Ts)
        if _is_plain_callable(dyn):        # closures as the reference takes them: traced into a device model (tracing.py)
            dyn, meas, _ = _trace_callables(dyn, meas, None, len(d0), nu, len(dg) if ny < 0 else ny, p)
            self.dynamics, self.measurement = dyn, meas
            nu = ny = -1
        if not isinstance(dyn, UserDynamics) and (isinstance(df, UserNoise) or isinstance(d0, UserInitial)):
            raise TypeError("UserNoise / UserInitial are members of a UserDynamics snippet")
        self._model = _build_model(dyn, meas, df, dg, d0, Ts, getattr(self, "_user_likelihood", False))
        self.nx, self.nu, self.ny = self._model.nx, self._model.nu, self._model.ny
        if nu not in (-1, self.nu) or ny not in (-1, self.ny):
            raise ValueError("nu / ny do not match the model descriptor")
        self._cfg = S.make_config(self._model, N, self.kind, resampling_strategy.code, resample_threshold, self.rng, device)
        self._h = _capi.FilterHandle(self._cfg)
        self.N = int(N)

    def set_parameters(self, *, dynamics=None, measurement=None, dynamics_density=None, measurement_density=None, initial_density=None):
        """New parameters for THIS filter (same model family and dimensions): what the reference's `filter_from_parameters(theta, pf)` is
        handed the old filter for (src/smoothing.jl:266-283) — nothing is reallocated on the device (llpf_set_model).  Returns self."""
        dyn = self.dynamics if dynamics is None else dynamics
        meas = self.measurement if measurement is None else measurement
        df = self.dynamics_density if dynamics_density is None else dynamics_density
        dg = self.measurement_density if measurement_density is None else measurement_density
        d0 = self.initial_density if initial_density is None else initial_density
        model = _build_model(dyn, meas, df, dg, d0, self.Ts, getattr(self, "_user_likelihood", False))
        self._h.set_model(model)
        self.dynamics, self.measurement, self.dynamics_density, self.measurement_density, self.initial_density = dyn, meas, df, dg, d0
        self._model = model
        return self

    # pf(u, y, p, t): one update! step (reference src/filtering.jl:238,240)
    def __call__(self, u, y, p=None, t=None):
        return update(self, u, y, p, t)

    @property
    def state(self):
        return _StateView(self)


class ParticleFilter(_AbstractParticleFilter):
    """ParticleFilter(N, dynamics, measurement, dynamics_density, measurement_density, initial_density; ...)
    — reference src/PFtypes.jl:21-36,65-75 (defaults: resample_threshold = 0.1, ResampleSystematic, Ts = 1)."""
    kind = S.PARTICLE_FILTER

    def __init__(self, N, dynamics, measurement, dynamics_density, measurement_density, initial_density, *,
                 resample_threshold=0.1, resampling_strategy=ResampleSystematic, rng=None, p=None,
                 threads=False, Ts=1.0, nu=-1, ny=-1, device=0):
        self._setup(N, dynamics, measurement, dynamics_density, measurement_density, initial_density,
                    resample_threshold, resampling_strategy, rng, p, threads, Ts, nu, ny, device)
        self.measurement_likelihood = None


class AdvancedParticleFilter(_AbstractParticleFilter):
    """AdvancedParticleFilter(N, dynamics, measurement, measurement_likelihood, dynamics_density,
    initial_density; ...) — reference src/PFtypes.jl:162-210 (default resample_threshold = 0.5)."""
    kind = S.ADVANCED_PARTICLE_FILTER

    def __init__(self, N, dynamics, measurement, measurement_likelihood, dynamics_density, initial_density, *,
                 resample_threshold=0.5, resampling_strategy=ResampleSystematic, rng=None, p=None,
                 threads=False, Ts=1.0, nu=-1, ny=-1, device=0, likelihood_bound=None):
        if _is_plain_callable(measurement_likelihood):      # measurement_likelihood(x, u, y, p, t) as a closure (src/PFtypes.jl:226-239)
            if not _is_plain_callable(dynamics) or ny < 0:
                raise TypeError("a callable measurement_likelihood needs callable dynamics / measurement and ny=")
            dynamics, measurement, measurement_likelihood = _trace_callables(dynamics, measurement, measurement_likelihood, len(initial_density), nu, ny, p,
                                                                             likelihood_bound)
            nu = -1
        self._user_likelihood = isinstance(measurement_likelihood, UserLikelihood)
        if isinstance(measurement_likelihood, UserLikelihood):
            if not isinstance(dynamics, UserDynamics):
                raise TypeError("a UserLikelihood is the loglik member of a UserDynamics snippet")
            dgs = MvNormal(np.zeros(dynamics.ny), 1.0)       # the descriptor's Gaussian is not used by such a model (its bound replaces the peak)
        elif isinstance(measurement_likelihood, GaussianLikelihood):
            dgs = measurement_likelihood.measurement_density
        else:
            raise TypeError("measurement_likelihood must be a GaussianLikelihood or a UserLikelihood descriptor")
        self._setup(N, dynamics, measurement, dynamics_density, dgs,
                    initial_density, resample_threshold, resampling_strategy, rng, p, threads, Ts, nu, ny, device)
        self.measurement_likelihood = measurement_likelihood


_DESCRIPTORS = (LinearDynamics, LinearMeasurement, QuadTankDynamics, QuadTankMeasurement, GaussianLikelihood, UserDynamics, UserMeasurement,
                UserLikelihood)


class KalmanFilter:
    """KalmanFilter(A, B, C, D, R1, R2, d0; Ts, device) — the reference's Kalman filter with constant matrices (src/kalman.jl):
    x' = A x + B u + w, w ~ N(0, R1);  y = C x + D u + e, e ~ N(0, R2);  x_0 ~ d0.  Runs on the device as a bank of one filter
    (llpf_kalman_bank_*), created on first use: as the inner filter of an RBPF it is a descriptor only (D = 0 there).
    R1, R2: matrices (a 1-D array: the diagonal; a float: sigma^2 I); d0: MvNormal.  nx <= 8, ny <= 4, nu <= 8."""
    _HANDLE = _capi.KalmanBankHandle          # the bank of one filter this class runs on

    def __init__(self, A, B, C, D, R1, R2, d0, *, Ts=1.0, device=0):
        self.A, self.B, self.C, self.D = np.atleast_2d(np.asarray(A, float)), B, C, D
        self.R1, self.R2, self.d0 = np.atleast_2d(np.asarray(R1, float)), np.atleast_2d(np.asarray(R2, float)), d0
        self._R1_in, self._R2_in = R1, R2
        self.Ts, self.device = float(Ts), int(device)
        self._handle = None

    def _model(self):
        """(llpf_model, D [ny, nu]) of this filter"""
        nx = self.A.shape[0]
        Cm = np.atleast_2d(np.asarray(self.C, float))
        ny = Cm.shape[0]
        B = np.zeros((nx, 0)) if self.B is None else np.asarray(self.B, float).reshape(nx, -1)
        nu = B.shape[1]
        cov = lambda c, n: MvNormal(np.zeros(n), c if np.ndim(c) < 2 else np.atleast_2d(np.asarray(c, float))).struct()
        d0 = self.d0.struct() if isinstance(self.d0, MvNormal) else self.d0
        m = S.make_lg_model(self.A, B, Cm, cov(self._R1_in, nx), cov(self._R2_in, ny), d0, self.Ts)
        D = np.broadcast_to(np.asarray(0.0 if self.D is None else self.D, float), (ny, nu)).copy()
        return m, D

    @property
    def _h(self):
        if self._handle is None:
            m, D = self._model()
            self._handle = self._HANDLE(self.device, [m], D[None])
        return self._handle

    @property
    def nx(self):
        return self.A.shape[0]

    @property
    def x(self):
        """state(kf): the current estimate"""
        return self._h.get_state()[0][0]

    @property
    def R(self):
        """covariance(kf)"""
        return self._h.get_state()[1][0]

    def _run(self, u, y, outputs=()):
        y = np.asarray(y, dtype=np.float64)
        y = y.reshape(y.shape[0], -1) if y.ndim else y.reshape(1, 1)
        r = self._h.run(None if self._h.nu == 0 else np.asarray(u, dtype=np.float64).reshape(y.shape[0], -1), y, outputs=outputs)
        return r


class SqKalmanFilter(KalmanFilter):
    """SqKalmanFilter(A, B, C, D, R1, R2, d0; Ts, device) — the reference's square-root Kalman filter (src/sq_kalman.jl): KalmanFilter's
    model and arguments, run on the device as a bank of one filter that carries a triangular factor of the covariance
    (llpf_sqkf_bank_*, csrc/shared/llpf_sqkf.h).  It stays finite where the covariance form loses positive definiteness (a diffuse prior
    with a near-perfect measurement).  R1, R2 and cov(d0) must be positive definite.  Every verb of a KalmanFilter applies except smooth;
    it is no inner filter of an RBPF and no mode of an IMM."""
    _HANDLE = _capi.SqkfBankHandle


class KalmanFilteringSolution:
    """Fields f, u, y, x, xt, R, Rt, ll, e, t of the reference's struct (src/solutions.jl): x, xt [T, nx] the prior and the posterior
    estimate of every step, R, Rt [T, nx, nx] their covariances, e [T, ny] the innovations (NaN at a missing measurement), ll the sum."""

    def __init__(self, f, u, y, x, xt, R, Rt, ll, e):
        self.f, self.u, self.y, self.x, self.xt, self.R, self.Rt, self.ll, self.e = f, u, y, x, xt, R, Rt, ll, e
        self.t = np.arange(x.shape[0]) * f.Ts


class KalmanSmoothingSolution(KalmanFilteringSolution):
    """The reference's KalmanSmoothingSolution (src/solutions.jl): the fields of the KalmanFilteringSolution it is built from, plus xT [T, nx]
    and RT [T, nx, nx], the mean and covariance of every state given all T measurements (the Rauch-Tung-Striebel smoother)."""

    def __init__(self, sol, xT, RT):
        super().__init__(sol.f, sol.u, sol.y, sol.x, sol.xt, sol.R, sol.Rt, sol.ll, sol.e)
        self.xT, self.RT = xT, RT


class IMM:
    """IMM(models, P, mu; interact, device) — the reference's interacting-multiple-model filter (src/imm.jl) over a list of KalmanFilter
    of the same dimensions, or over a list of ExtendedKalmanFilter or a list of UnscentedKalmanFilter of ONE model (the same compiled model
    id and dimensions; the modes differ by their parameters, R1, R2 and d0 — a snippet that needs structurally different modes branches on
    one of its parameters):
    P [M, M] the row-stochastic transition matrix (P[i, j]: from mode i to mode j), mu [M] the initial mode probabilities, M <= 4.  Runs on
    the device as a bank of one IMM (llpf_imm_bank_*), created on first use, in the operation order of csrc/shared/llpf_imm.h: the
    textbook recursion of Blom & Bar-Shalom, not checked against the reference's source.  An extended mode linearises its measurement at
    its own prior and its dynamics at its own state after the mixing (csrc/shared/llpf_ekf.h).  An unscented mode is the additive-noise
    unscented Kalman filter (csrc/shared/llpf_ukf.h): it maps the 2 nx + 1 sigma points of its own prior through the measurement and those
    of its own state after the mixing through the dynamics, so its model needs no Jacobians (a snippet without dynamics_jac /
    measurement_jac, a callable traced without them); all modes carry the same `weights`, the one set of the bank.  `unscented`: the
    modes are unscented Kalman filters; `extended`: they are extended Kalman filters.  Iterated modes, and modes of different kinds in
    one IMM, are not provided.  interact = False: the modes never mix (M independent filters with a shared mode probability).  There is no smoother."""

    def __init__(self, models, P, mu, *, interact=True, device=0):
        self.models = list(models)
        if not self.models:
            raise TypeError("IMM: models is a non-empty list of KalmanFilter, of ExtendedKalmanFilter or of UnscentedKalmanFilter")
        kinds = []
        for j, m in enumerate(self.models):
            if isinstance(m, SqKalmanFilter):
                raise TypeError("IMM: the modes are KalmanFilter, ExtendedKalmanFilter or UnscentedKalmanFilter; mode %d is a SqKalmanFilter" % j)
            kind = ("linear" if isinstance(m, KalmanFilter) else "unscented" if isinstance(m, UnscentedKalmanFilter)
                    else "extended" if isinstance(m, ExtendedKalmanFilter) and not isinstance(m, IteratedExtendedKalmanFilter) else None)
            if kind is None:
                raise TypeError("IMM: models is a list of KalmanFilter, of ExtendedKalmanFilter or of UnscentedKalmanFilter; mode %d is a %s"
                                % (j, type(m).__name__))
            kinds.append(kind)
        for j, kind in enumerate(kinds):
            if kind != kinds[0]:
                raise TypeError("IMM: the modes of one IMM are one kind of filter; mode 0 is a %s and mode %d a %s"
                                % (type(self.models[0]).__name__, j, type(self.models[j]).__name__))
        self.kind = kinds[0]      # "linear", "extended" or "unscented"
        self.weights = None
        if self._timed:
            m0 = self.models[0]._model
            for j, f in enumerate(self.models):
                m = f._model
                if (m.model_id, m.nx, m.ny, m.nu) != (m0.model_id, m0.nx, m0.ny, m0.nu):
                    raise TypeError("IMM: the modes of an %s IMM are one model (the same compiled model id and dimensions); mode %d "
                                    "differs from mode 0" % (kinds[0], j))
        if self.unscented:
            self.weights = self.models[0].weights
            for j, f in enumerate(self.models):
                if f.weights != self.weights:
                    raise TypeError("IMM: mode %d has other weights (gamma, wm0, wc0, wi) than mode 0; an unscented IMM has one set" % j)
        self.P, self.mu0 = np.atleast_2d(np.asarray(P, float)), np.atleast_1d(np.asarray(mu, float))
        self.interact, self.device = bool(interact), int(device)
        self.Ts = self.models[0].Ts
        self._handle = None
        self._index = 0         # extended, unscented: the step counter of the nonlinear filters (the time of update!'s step)

    @property
    def extended(self):
        """the modes are extended Kalman filters"""
        return self.kind == "extended"

    @property
    def unscented(self):
        """the modes are unscented Kalman filters"""
        return self.kind == "unscented"

    @property
    def _timed(self):
        """the modes are driven by a model's own functions and take a time: extended or unscented"""
        return self.kind != "linear"

    def _spec(self):
        """(models [M], D [M, ny, nu] or None (extended, unscented), P, mu0) of this filter"""
        if self._timed:
            return [f._model for f in self.models], None, self.P, self.mu0
        md = [kf._model() for kf in self.models]
        return [m for m, _ in md], np.stack([D for _, D in md]), self.P, self.mu0

    @property
    def _h(self):
        if self._handle is None:
            models, D, P, mu0 = self._spec()
            self._handle = _capi.IMMBankHandle(self.device, [models], None if D is None else D[None], P[None], mu0[None], self.interact,
                                               self.extended, self.unscented, self.weights)
        return self._handle

    @property
    def nx(self):
        return self.models[0].nx

    @property
    def x(self):
        """state(imm): the combined estimate sum_j mu_j x_j"""
        return self._h.get_state()[0][0]

    @property
    def R(self):
        """covariance(imm): the combined covariance sum_j mu_j (R_j + (x_j - x)(x_j - x)')"""
        return self._h.get_state()[1][0]

    @property
    def mu(self):
        """the current mode probabilities [M]"""
        return self._h.get_modes()[2][0]

    def reset(self):
        self._h.reset()
        self._index = 1         # index(pf) after reset!, as the nonlinear filters count it

    def _run(self, u, y, outputs=(), t_index0=0.0):
        y = np.asarray(y, dtype=np.float64)
        y = y.reshape(y.shape[0], -1) if y.ndim else y.reshape(1, 1)
        r = self._h.run(None if self._h.nu == 0 else np.asarray(u, dtype=np.float64).reshape(y.shape[0], -1), y, outputs=outputs,
                        t_index0=t_index0)
        self._index += y.shape[0]
        return r


class IMMFilteringSolution(KalmanFilteringSolution):
    """forward_trajectory(imm, u, y): the fields of a KalmanFilteringSolution for the combined estimate (e is None: an IMM has one
    innovation per mode), plus mu [T, M], the posterior mode probabilities, and ll_modes [T, M], every mode's own log-likelihood."""

    def __init__(self, f, u, y, x, xt, R, Rt, ll, mu, ll_modes):
        super().__init__(f, u, y, x, xt, R, Rt, ll, None)
        self.mu, self.ll_modes = mu, ll_modes


def covariance(kf):
    """covariance(kf) — the covariance R of the current estimate of a KalmanFilter, an UnscentedKalmanFilter, an ExtendedKalmanFilter or an
    EnsembleKalmanFilter (its sample covariance)"""
    return kf.R


class _KfBank:
    """What KalmanFilterBank, UnscentedKalmanFilterBank and ExtendedKalmanFilterBank share: a bank handle `_h` of one GPU thread per filter.  `_AT_LOGLIK` and
    `_AT_FORWARD` are the keyword arguments the handle's run / smooth take for the time of the first step."""
    _AT_LOGLIK = _AT_FORWARD = {}

    def reset(self):
        self._h.reset()

    def state(self):
        """(x [F, nx], R [F, nx, nx]) of every filter"""
        return self._h.get_state()

    def _io(self, u, y):
        y = np.asarray(y, dtype=np.float64)
        y_per = y.ndim == 3
        if self._h.nu == 0 or u is None:
            return None, False, y, y_per
        u = np.asarray(u, dtype=np.float64)
        return u, u.ndim == 3, y, y_per

    def loglik(self, u, y):
        """[loglik(f_k, u, y) for k]: reset, then T update! steps (those of an unscented bank the first at t = 1 * Ts as FilterBank.loglik).
        u [T, nu] / y [T, ny] shared, or [F, T, n] per filter (by ndim)."""
        u, up, y, yp = self._io(u, y)
        self._h.reset()
        return self._h.run(u, y, up, yp, **self._AT_LOGLIK)["ll"]

    def forward(self, u, y, outputs=_capi.KALMAN_OUTPUTS):
        """forward_trajectory of every filter (the first step at t = 0): {"ll": [F], "ll_steps": [T, F], "x", "xt": [T, F, nx], "R", "Rt":
        [T, F, nx, nx], "e": [T, F, ny]} for the names in `outputs`"""
        u, up, y, yp = self._io(u, y)
        self._h.reset()
        return self._h.run(u, y, up, yp, outputs=outputs, **self._AT_FORWARD)

    def smooth(self, u, y, outputs=_capi.KALMAN_SMOOTH_OUTPUTS, forward=()):
        """smooth(f_k, u, y) of every filter (reset, the forward pass of forward(), the RTS smoother — an unscented bank's the unscented one —
        on the device): {"ll": [F], "xT": [T, F, nx], "RT": [T, F, nx, nx]} for the names in `outputs`, plus the forward outputs named in
        `forward` (as forward())"""
        u, up, y, yp = self._io(u, y)
        self._h.reset()
        return self._h.smooth(u, y, up, yp, outputs=outputs, forward=forward, **self._AT_FORWARD)


class KalmanFilterBank(_KfBank):
    """n independent Kalman filters with constant matrices of the same dimensions on one device, one GPU thread each
    (llpf_kalman_bank_*): the exact log-likelihood of every parameter set of a linear-Gaussian sweep.  `filters_spec` is a list of
    KalmanFilter or of (A, B, C, D, R1, R2, d0) tuples."""
    _HANDLE = _capi.KalmanBankHandle

    def __init__(self, filters_spec, device=0):
        models, Ds = self._models(filters_spec)
        self.device = int(device)
        self._h = self._HANDLE(self.device, models, Ds)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)

    @staticmethod
    def _models(filters_spec):
        kfs = [f if isinstance(f, KalmanFilter) else KalmanFilter(*f) for f in filters_spec]
        md = [kf._model() for kf in kfs]
        return [m for m, _ in md], np.stack([D for _, D in md])

    @classmethod
    def from_filter_bank(cls, bank, device=None):
        """the Kalman twin of a FilterBank of linear-Gaussian filters: the same descriptors, D = 0"""
        self = cls.__new__(cls)
        models = list(bank._models)
        if any(m.model_id != S.MODEL_LINEAR_GAUSSIAN for m in models):
            raise TypeError("from_filter_bank: every filter of the bank must be linear-Gaussian")
        self.device = int(bank._h.cfg.device if device is None else device)
        self._h = cls._HANDLE(self.device, models, None)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)
        return self

    def set_parameters(self, filters_spec):
        """new matrices for every filter (same dimensions, nothing reallocated: llpf_kalman_bank_set_models)"""
        models, Ds = self._models(filters_spec)
        self._h.set_models(models, Ds)


class SqKalmanFilterBank(KalmanFilterBank):
    """n independent square-root Kalman filters on one device, one GPU thread each (llpf_sqkf_bank_*): KalmanFilterBank's constructor,
    from_filter_bank, loglik, forward, state and set_parameters, for sweeps whose noise levels span so many decades that the covariance
    form loses positive definiteness.  `filters_spec` is a list of KalmanFilter, SqKalmanFilter or (A, B, C, D, R1, R2, d0) tuples.
    There is no smoother."""
    _HANDLE = _capi.SqkfBankHandle

    def smooth(self, *args, **kwargs):
        raise TypeError("the square-root Kalman filter has no smoother")


class IMMBank(_KfBank):
    """n independent IMM filters of the same number of modes and the same dimensions on one device, one GPU lane per (filter, mode)
    (llpf_imm_bank_*): the exact log-likelihood of a switching linear-Gaussian model for every parameter set of a sweep, or, over
    ExtendedKalmanFilter modes of one model, the first-order one of a switching nonlinear model, or, over UnscentedKalmanFilter modes of
    one model and one set of weights (a model without Jacobians), the unscented one.  `specs` is a list of IMM or of
    (models, P, mu) tuples (all with the same `interact`, the first one's, and all over the same kind of mode).  An extended or unscented
    bank runs loglik from t = 1 * Ts and forward from t = 0, as ExtendedKalmanFilterBank does.  Iterated modes are not provided."""

    def __init__(self, specs, device=0):
        models, D, P, mu0, interact, self.kind, self.weights = self._tables(specs)
        self.device = int(device)
        self._h = _capi.IMMBankHandle(self.device, models, D, P, mu0, interact, self.extended, self.unscented, self.weights)
        self.n_filters = len(models)
        self.Ts = float(models[0][0].Ts)
        if self.kind != "linear":
            self._AT_LOGLIK, self._AT_FORWARD = {"t_index0": 1.0}, {"t_index0": 0.0}

    extended = property(lambda self: self.kind == "extended", doc="the modes are extended Kalman filters")
    unscented = property(lambda self: self.kind == "unscented", doc="the modes are unscented Kalman filters")

    @staticmethod
    def _tables(specs):
        """(models, D, P, mu0, interact, kind, weights) of the specs, every IMM built once: one kind of mode (IMM.kind; D None unless it is
        "linear") and, of an unscented bank, one set of weights (None otherwise)"""
        imms = [f if isinstance(f, IMM) else IMM(*f) for f in specs]
        kind, weights = imms[0].kind, imms[0].weights
        for k, f in enumerate(imms):
            if f.kind != kind:
                raise TypeError("IMMBank: filter %d is %s where filter 0 is %s: a bank is over one kind of mode" % (k, f.kind, kind))
            if f.weights != weights:
                raise TypeError("IMMBank: filter %d has other weights than filter 0: an unscented bank has one set" % k)
        sp = [f._spec() for f in imms]
        D = np.stack([s[1] for s in sp]) if kind == "linear" else None
        return [s[0] for s in sp], D, np.stack([s[2] for s in sp]), np.stack([s[3] for s in sp]), imms[0].interact, kind, weights

    @staticmethod
    def _pack(specs):
        """(models, D, P, mu0, interact, extended) of the specs"""
        t = IMMBank._tables(specs)
        return t[:5] + (t[5] == "extended",)

    def state(self):
        """(x [F, nx], R [F, nx, nx], mu [F, M]): the combined estimate and the mode probabilities of every filter"""
        return self._h.get_modes()[:3]

    def forward(self, u, y, outputs=_capi.IMM_OUTPUTS):
        """forward_trajectory of every filter: {"ll": [F], "ll_steps": [T, F], "x", "xt": [T, F, nx], "R", "Rt": [T, F, nx, nx], "mu",
        "ll_modes": [T, F, M]} for the names in `outputs`"""
        return super().forward(u, y, outputs)

    def smooth(self, u=None, y=None, outputs=None, forward=()):
        raise TypeError("the IMM filter has no smoother")

    def set_parameters(self, specs):
        """new matrices, P and mu for every filter (same shapes, nothing reallocated: llpf_imm_bank_set_models)"""
        models, D, P, mu0, _, kind, weights = self._tables(specs)
        if kind != self.kind:
            raise TypeError("IMMBank.set_parameters: the bank keeps its kind of mode")
        self._h.set_models(models, D, P, mu0)
        if weights != self.weights:
            self._h.set_weights(weights)
            self.weights = weights


class MerweParams:
    """MerweParams(alpha, beta, kappa) — the scaled unscented transform of Van der Merwe.  With L = nx:
    lambda = alpha^2 (L + kappa) - L,  gamma = sqrt(L + lambda),  wm0 = lambda / (L + lambda),  wc0 = wm0 + 1 - alpha^2 + beta,
    wi = 1 / (2 (L + lambda)).  Defaults (1e-3, 2, 0): unverified against the reference (no source here)."""

    def __init__(self, alpha=1e-3, beta=2.0, kappa=0.0):
        self.alpha, self.beta, self.kappa = float(alpha), float(beta), float(kappa)

    def weights(self, L):
        a2 = self.alpha * self.alpha
        lam = a2 * (L + self.kappa) - L
        wm0 = lam / (L + lam)
        return float(np.sqrt(L + lam)), wm0, wm0 + 1.0 - a2 + self.beta, 1.0 / (2.0 * (L + lam))


class WikiParams:
    """WikiParams(alpha, beta, kappa) — the parametrisation of the Wikipedia article on the Kalman filter.  With L = nx:
    gamma = alpha sqrt(kappa),  wm0 = (alpha^2 kappa - L) / (alpha^2 kappa),  wc0 = wm0 + 1 - alpha^2 + beta,  wi = 1 / (2 alpha^2 kappa).
    Defaults (1, 0, 1): unverified against the reference (no source here)."""

    def __init__(self, alpha=1.0, beta=0.0, kappa=1.0):
        self.alpha, self.beta, self.kappa = float(alpha), float(beta), float(kappa)

    def weights(self, L):
        a2k = self.alpha * self.alpha * self.kappa
        wm0 = (a2k - L) / a2k
        return float(self.alpha * np.sqrt(self.kappa)), wm0, wm0 + 1.0 - self.alpha * self.alpha + self.beta, 1.0 / (2.0 * a2k)


class TrivialParams:
    """TrivialParams() — every one of the 2 L + 1 points carries the same weight: wm0 = wc0 = wi = 1 / (2 L + 1), gamma = sqrt(L + 1/2)
    (so that wi gamma^2 = 1/2: mean and covariance of a linear map are exact).  The default of UnscentedKalmanFilter.  Name and default
    follow the reference's documentation; the formula is unverified against the reference (no source here)."""

    def weights(self, L):
        w = 1.0 / (2.0 * L + 1.0)
        return float(np.sqrt(L + 0.5)), w, w, w


def _ukf_weights(weight_params, L):
    """(gamma, wm0, wc0, wi) from a preset (an object with weights(L)), a raw 4-tuple, or None (TrivialParams)"""
    if weight_params is None:
        weight_params = TrivialParams()
    if hasattr(weight_params, "weights"):
        return tuple(float(v) for v in weight_params.weights(int(L)))
    w = tuple(float(v) for v in weight_params)
    if len(w) != 4:
        raise ValueError("weight_params: a preset (MerweParams, WikiParams, TrivialParams) or the four numbers (gamma, wm0, wc0, wi)")
    return w


class _NonlinearKalmanFilter:
    """What UnscentedKalmanFilter and ExtendedKalmanFilter share: the model descriptor of (dynamics, measurement, R1, R2, d0) and a bank of
    one filter on the device, created on first use by `_open()`.  `_JACOBIANS`: plain callables are traced with their Jacobians."""
    _JACOBIANS = False
    _NOISE_INPUT = False      # a plain callable dynamics of five parameters (x, u, p, t, w) is traced into dynamics_w as well

    def _setup(self, dynamics, measurement, R1, R2, d0, Ts, nu, ny, p, device):
        nx = len(d0)
        if ny < 0 and np.ndim(R2) >= 1:
            ny = np.asarray(R2).shape[0]
        if _is_plain_callable(dynamics):
            if ny < 0:
                raise ValueError("pass ny= with callable dynamics and a scalar R2")
            from . import tracing
            dynamics, measurement, _ = _trace_callables(dynamics, measurement, None, nx, nu, ny, p, jacobians=self._JACOBIANS,
                                                        noise_input=self._NOISE_INPUT and tracing.n_parameters(dynamics) == 5)
        if isinstance(dynamics, UserDynamics):
            ny = dynamics.ny
        elif isinstance(measurement, LinearMeasurement):
            ny = measurement.C.shape[0]
        elif isinstance(measurement, QuadTankMeasurement):
            ny = 2
        cov = lambda c, n: MvNormal(np.zeros(n), c if np.ndim(c) < 2 else np.atleast_2d(np.asarray(c, float)))
        self.dynamics, self.measurement, self.R1, self.R2, self.d0 = dynamics, measurement, R1, R2, d0
        self.dynamics_density, self.measurement_density, self.initial_density = cov(R1, nx), cov(R2, ny), d0
        self.p, self.Ts, self.device = p, float(Ts), int(device)
        self._model = _build_model(dynamics, measurement, self.dynamics_density, self.measurement_density, d0, Ts)
        self.nx, self.nu, self.ny = self._model.nx, self._model.nu, self._model.ny
        self._handle = None
        self._index = 0

    @property
    def _h(self):
        if self._handle is None:
            self._handle = self._open()
        return self._handle

    @property
    def x(self):
        """state(kf): the current estimate"""
        return self._h.get_state()[0][0]

    @property
    def R(self):
        """covariance(kf)"""
        return self._h.get_state()[1][0]

    def reset(self):
        self._h.reset()
        self._index = 1         # index(pf) after reset!, as the particle filters count it

    def _run(self, u, y, outputs=(), t_index0=0.0):
        y = np.asarray(y, dtype=np.float64)
        y = y.reshape(y.shape[0], -1) if y.ndim else y.reshape(1, 1)
        u = None if self.nu == 0 else np.asarray(u, dtype=np.float64).reshape(y.shape[0], -1)
        r = self._h.run(u, y, outputs=outputs, t_index0=t_index0)
        self._index += y.shape[0]
        return r

    def _step(self, u, y, t, outputs):
        """one step at time t (default index * Ts): y None is a missing measurement"""
        t0 = float(self._index) if t is None else float(t) / self.Ts
        yr = np.full((1, self.ny), np.nan) if y is None else np.atleast_1d(np.asarray(y, float))[None]
        ur = np.zeros((1, max(self.nu, 1))) if u is None else np.atleast_1d(np.asarray(u, float))[None]
        return self._run(ur, yr, outputs, t0)

    def __call__(self, u, y, p=None, t=None):
        return update(self, u, y, p, t)


class UnscentedKalmanFilter(_NonlinearKalmanFilter):
    """UnscentedKalmanFilter(dynamics, measurement, R1, R2, d0; Ts, nu, ny, p, weight_params, device) — the reference's unscented Kalman
    filter with additive noise: x' = f(x, u, p, t) + w, w ~ N(0, R1);  y = g(x, u, p, t) + e, e ~ N(0, R2);  x_0 ~ d0 (csrc/shared/llpf_ukf.h
    is the definition).  `dynamics` / `measurement` are what a ParticleFilter takes: LinearDynamics + LinearMeasurement, QuadTankDynamics +
    QuadTankMeasurement, UserDynamics + UserMeasurement, or a pair of plain callables (traced: tracing.py; pass nu=, and ny= unless R2 is
    a matrix).  R1, R2: matrices (a 1-D array: the diagonal; a float: sigma^2 I); d0: MvNormal.  weight_params: MerweParams, WikiParams,
    TrivialParams (the default) or the four numbers (gamma, wm0, wc0, wi).  Runs on the device as a bank of one filter (llpf_ukf_bank_*),
    created on first use.  nx <= 8, ny <= 4, nu <= 8."""

    def __init__(self, dynamics, measurement, R1, R2, d0, *, Ts=1.0, nu=-1, ny=-1, p=None, weight_params=None, device=0):
        self._setup(dynamics, measurement, R1, R2, d0, Ts, nu, ny, p, device)
        self.weight_params = weight_params
        self.weights = _ukf_weights(weight_params, self.nx)

    def _open(self):
        return _capi.UkfBankHandle(self.device, [self._model], self.weights)


def _aukf_weights(weight_params, nx):
    """the pair (measurement set for L = nx, dynamics set for L = 2 nx), each (gamma, wm0, wc0, wi): from a preset (an object with
    weights(L)), None (TrivialParams), or a pair of 4-tuples; one 4-tuple cannot say both"""
    if weight_params is None:
        weight_params = TrivialParams()
    if hasattr(weight_params, "weights"):
        return _ukf_weights(weight_params, nx), _ukf_weights(weight_params, 2 * nx)
    pair = tuple(weight_params)
    if len(pair) != 2 or any(np.ndim(w) != 1 or len(w) != 4 for w in pair):
        raise ValueError("weight_params: a preset (MerweParams, WikiParams, TrivialParams) or a pair of four numbers (gamma, wm0, wc0, wi), "
                         "the measurement set (L = nx) and the dynamics set (L = 2 nx)")
    return tuple(_ukf_weights(w, nx) for w in pair)


class AugmentedUnscentedKalmanFilter(_NonlinearKalmanFilter):
    """AugmentedUnscentedKalmanFilter(dynamics, measurement, R1, R2, d0; Ts, nu, ny, p, weight_params, device) — the unscented Kalman
    filter with augmented (non-additive) process noise, the reference's UnscentedKalmanFilter with dynamics(x, u, p, t, w):
    x' = f(x, u, p, t, w), w in R^nx, w ~ N(0, R1);  y = g(x, u, p, t) + e, e ~ N(0, R2);  x_0 ~ d0 (csrc/shared/llpf_aukf.h is the
    definition: predict! maps 4 nx + 1 points of (x; w), correct! is the UnscentedKalmanFilter's).  The arguments are
    UnscentedKalmanFilter's.  A plain callable dynamics with five parameters (x, u, p, t, w) is traced into the model's `dynamics_w`
    member (and, at w = 0, into `dynamics`); a UserDynamics snippet defines the member itself; a model without it (every built-in
    descriptor, a callable of four parameters) is taken as additive, f(x) + w.  weight_params: a preset, used at L = nx for the measurement
    and at L = 2 nx for the dynamics, or a pair of (gamma, wm0, wc0, wi).  Runs on the device as a bank of one filter (llpf_aukf_bank_*),
    created on first use.  There is no smoother, and the filter is not a mode of an IMM."""
    _NOISE_INPUT = True

    def __init__(self, dynamics, measurement, R1, R2, d0, *, Ts=1.0, nu=-1, ny=-1, p=None, weight_params=None, device=0):
        self._setup(dynamics, measurement, R1, R2, d0, Ts, nu, ny, p, device)
        self.weight_params = weight_params
        self.weights = _aukf_weights(weight_params, self.nx)

    def _open(self):
        return _capi.AukfBankHandle(self.device, [self._model], self.weights)


class ExtendedKalmanFilter(_NonlinearKalmanFilter):
    """ExtendedKalmanFilter(dynamics, measurement, R1, R2, d0; Ts, nu, ny, p, device) — the first-order extended Kalman filter with
    additive noise: x' = f(x, u, p, t) + w, w ~ N(0, R1);  y = g(x, u, p, t) + e, e ~ N(0, R2);  x_0 ~ d0; correct! linearises g at the
    prior mean, predict! linearises f at the posterior mean (csrc/shared/llpf_ekf.h is the definition).  The arguments are
    UnscentedKalmanFilter's.  The Jacobians come from the model: the built-in descriptors have them, a pair of plain callables is traced
    and differentiated in forward mode (tracing.py, jacobians=True), and a UserDynamics snippet must define the members
    `dynamics_jac(x, fx, J)` and `measurement_jac(x, gx, J)` itself.  Runs on the device as a bank of one filter (llpf_ekf_bank_*), created
    on first use.  nx <= 8, ny <= 4, nu <= 8."""
    _JACOBIANS = True

    def __init__(self, dynamics, measurement, R1, R2, d0, *, Ts=1.0, nu=-1, ny=-1, p=None, device=0):
        self._setup(dynamics, measurement, R1, R2, d0, Ts, nu, ny, p, device)
        _need_jacobians(self._model)

    def _open(self):
        return _capi.EkfBankHandle(self.device, [self._model])


class IteratedExtendedKalmanFilter(ExtendedKalmanFilter):
    """IteratedExtendedKalmanFilter(dynamics, measurement, R1, R2, d0; maxiters=10, epsilon=1e-8, Ts, nu, ny, p, device) — the iterated
    extended Kalman filter: ExtendedKalmanFilter whose correct! is a Gauss-Newton iteration that moves the linearisation point of g from
    the prior mean towards the posterior mode, at most `maxiters` linearisations per step, stopped once no state moved by more than
    `epsilon` (csrc/shared/llpf_ekf.h: llpf_iekf_iterate is the definition; the full step, no step length).  predict! is the extended
    filter's, and maxiters=1 is that filter bit for bit.  ll, e, xt and Rt of a step are those of its last linearisation."""

    def __init__(self, dynamics, measurement, R1, R2, d0, *, maxiters=10, epsilon=1e-8, Ts=1.0, nu=-1, ny=-1, p=None, device=0):
        super().__init__(dynamics, measurement, R1, R2, d0, Ts=Ts, nu=nu, ny=ny, p=p, device=device)
        self.maxiters, self.epsilon = int(maxiters), float(epsilon)

    def _open(self):
        h = super()._open()
        h.set_iterations(self.maxiters, self.epsilon)
        return h


class SqExtendedKalmanFilter(_NonlinearKalmanFilter):
    """SqExtendedKalmanFilter(dynamics, measurement, R1, R2, d0; Ts, nu, ny, p, device) — the square-root extended Kalman filter:
    ExtendedKalmanFilter's arguments, model, verbs and time conventions, carrying a lower-triangular factor L of the covariance, R = L L'
    (csrc/shared/llpf_sqekf.h is the definition: predict! triangularises [L1 | A L], correct! [[L2, C L], [0, L]] by Householder
    reflections, with the Jacobians A and C of the model at the current mean).  No covariance is ever subtracted from, so a diffuse prior
    with a near-exact sensor, which turns an ExtendedKalmanFilter NaN, stays finite.  R1, R2 and cov(d0) must be positive definite.
    Runs on the device as a bank of one filter (llpf_sqekf_bank_*), created on first use.  correct! alone puts the posterior back through
    its covariance (factored again); update! and forward_trajectory carry the factor itself.  There is no smoother and no iterated
    form, and the filter is not a mode of an IMM."""
    _JACOBIANS = True

    def __init__(self, dynamics, measurement, R1, R2, d0, *, Ts=1.0, nu=-1, ny=-1, p=None, device=0):
        self._setup(dynamics, measurement, R1, R2, d0, Ts, nu, ny, p, device)
        _need_jacobians(self._model)

    def _open(self):
        return _capi.SqekfBankHandle(self.device, [self._model])


def _need_jacobians(model):
    """a compiled model under an extended Kalman filter must define both Jacobian members"""
    if model.model_id < S.MODEL_USER_BASE:
        return
    traits = _capi.model_traits(model.model_id)
    missing = [name for name, bit in (("dynamics_jac", _capi.TRAIT_DYNAMICS_JAC), ("measurement_jac", _capi.TRAIT_MEASUREMENT_JAC)) if not traits & bit]
    if missing:
        raise TypeError("an ExtendedKalmanFilter needs the model's Jacobians: the snippet defines no `%s` member "
                        "(DEV void dynamics_jac(const double* x, double* fx, double* J) const, measurement_jac likewise)" % "`, `".join(missing))


class UnscentedKalmanFilterBank(_KfBank):
    """n independent unscented Kalman filters of the same model family and dimensions on one device, one GPU thread each
    (llpf_ukf_bank_*): the deterministic log-likelihood of every parameter set of a nonlinear sweep.  `filters_spec` is a list of
    UnscentedKalmanFilter or of (dynamics, measurement, R1, R2, d0) tuples; `weight_params` as UnscentedKalmanFilter takes them, one set
    for the bank."""
    _AT_LOGLIK, _AT_FORWARD = {"t_index0": 1.0}, {"t_index0": 0.0}

    def __init__(self, filters_spec, device=0, weight_params=None, Ts=1.0):
        models = self._models(filters_spec, Ts)
        self._init(models, device, weight_params)

    def _init(self, models, device, weight_params):
        self.device = int(device)
        self.weights = _ukf_weights(weight_params, models[0].nx)
        self._h = _capi.UkfBankHandle(self.device, models, self.weights)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)

    @staticmethod
    def _models(filters_spec, Ts):
        return [(f if isinstance(f, UnscentedKalmanFilter) else UnscentedKalmanFilter(*f, Ts=Ts))._model for f in filters_spec]

    @classmethod
    def from_filter_bank(cls, bank, device=None, weight_params=None):
        """the unscented twin of a FilterBank: the same descriptors (any model that is not Rao-Blackwellized and keeps the Gaussian
        densities), loglik and forward at the times FilterBank.loglik and FilterBank.forward use"""
        self = cls.__new__(cls)
        self._init(list(bank._models), bank._h.cfg.device if device is None else device, weight_params)
        return self

    def set_parameters(self, filters_spec):
        """new parameters for every filter (same model and dimensions, nothing reallocated: llpf_ukf_bank_set_models)"""
        self._h.set_models(self._models(filters_spec, self.Ts))

    def set_weights(self, weight_params):
        self.weights = _ukf_weights(weight_params, self._h.nx)
        self._h.set_weights(self.weights)


class AugmentedUnscentedKalmanFilterBank(_KfBank):
    """n independent unscented Kalman filters with augmented process noise of the same model family and dimensions on one device, one GPU
    thread each (llpf_aukf_bank_*): the log-likelihood, free of Monte-Carlo noise, of every parameter set of a sweep over a model whose
    process noise is not additive.  `filters_spec` is a list of AugmentedUnscentedKalmanFilter or of (dynamics, measurement, R1, R2, d0)
    tuples; `weight_params` as AugmentedUnscentedKalmanFilter takes them, one pair of sets for the bank.  There is no smoother."""
    _AT_LOGLIK, _AT_FORWARD = {"t_index0": 1.0}, {"t_index0": 0.0}

    def __init__(self, filters_spec, device=0, weight_params=None, Ts=1.0):
        self._init(self._models(filters_spec, Ts), device, weight_params)

    def _init(self, models, device, weight_params):
        self.device = int(device)
        self.weights = _aukf_weights(weight_params, models[0].nx)
        self._h = _capi.AukfBankHandle(self.device, models, self.weights)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)

    @staticmethod
    def _models(filters_spec, Ts):
        return [(f if isinstance(f, AugmentedUnscentedKalmanFilter) else AugmentedUnscentedKalmanFilter(*f, Ts=Ts))._model for f in filters_spec]

    @classmethod
    def from_filter_bank(cls, bank, device=None, weight_params=None):
        """the augmented unscented twin of a FilterBank: the same descriptors (any model that is not Rao-Blackwellized and keeps the
        Gaussian densities), loglik and forward at the times FilterBank.loglik and FilterBank.forward use"""
        self = cls.__new__(cls)
        self._init(list(bank._models), bank._h.cfg.device if device is None else device, weight_params)
        return self

    def set_parameters(self, filters_spec):
        """new parameters for every filter (same model and dimensions, nothing reallocated: llpf_aukf_bank_set_models)"""
        self._h.set_models(self._models(filters_spec, self.Ts))

    def set_weights(self, weight_params):
        self.weights = _aukf_weights(weight_params, self._h.nx)
        self._h.set_weights(self.weights)

    def smooth(self, *args, **kwargs):
        raise TypeError("the augmented unscented Kalman filter has no smoother")


class ExtendedKalmanFilterBank(_KfBank):
    """n independent extended Kalman filters of the same model family and dimensions on one device, one GPU thread each
    (llpf_ekf_bank_*): the deterministic log-likelihood of every parameter set of a nonlinear sweep at one evaluation of the model and
    its Jacobian per stage.  `filters_spec` is a list of ExtendedKalmanFilter or of (dynamics, measurement, R1, R2, d0) tuples."""
    _AT_LOGLIK, _AT_FORWARD = {"t_index0": 1.0}, {"t_index0": 0.0}
    _HANDLE = _capi.EkfBankHandle

    def __init__(self, filters_spec, device=0, Ts=1.0):
        self._init(self._models(filters_spec, Ts), device)

    def _init(self, models, device):
        self.device = int(device)
        for m in models:
            _need_jacobians(m)
        self._h = self._HANDLE(self.device, models)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)

    @staticmethod
    def _models(filters_spec, Ts):
        return [(f if isinstance(f, ExtendedKalmanFilter) else ExtendedKalmanFilter(*f, Ts=Ts))._model for f in filters_spec]

    @classmethod
    def from_filter_bank(cls, bank, device=None):
        """the extended twin of a FilterBank: the same descriptors (any model that is not Rao-Blackwellized, keeps the Gaussian densities
        and has its Jacobians), loglik and forward at the times FilterBank.loglik and FilterBank.forward use"""
        self = cls.__new__(cls)
        self._init(list(bank._models), bank._h.cfg.device if device is None else device)
        return self

    def set_parameters(self, filters_spec):
        """new parameters for every filter (same model and dimensions, nothing reallocated: llpf_ekf_bank_set_models)"""
        self._h.set_models(self._models(filters_spec, self.Ts))

    def smooth(self, u, y, outputs=None, forward=()):
        raise TypeError("the extended Kalman filter has no smoother yet: use UnscentedKalmanFilterBank.smooth")


class SqExtendedKalmanFilterBank(ExtendedKalmanFilterBank):
    """n independent square-root extended Kalman filters on one device, one GPU thread each (llpf_sqekf_bank_*):
    ExtendedKalmanFilterBank's constructor, from_filter_bank, loglik, forward, state, set_parameters and time conventions, for nonlinear
    sweeps whose noise levels span so many decades that the covariance form loses positive definiteness.  `filters_spec` is a list of
    SqExtendedKalmanFilter, ExtendedKalmanFilter or (dynamics, measurement, R1, R2, d0) tuples.  There is no smoother."""
    _HANDLE = _capi.SqekfBankHandle

    @staticmethod
    def _models(filters_spec, Ts):
        return [(f if isinstance(f, (SqExtendedKalmanFilter, ExtendedKalmanFilter)) else SqExtendedKalmanFilter(*f, Ts=Ts))._model for f in filters_spec]

    def smooth(self, *args, **kwargs):
        raise TypeError("the square-root extended Kalman filter has no smoother")


class IteratedExtendedKalmanFilterBank(ExtendedKalmanFilterBank):
    """n independent iterated extended Kalman filters on one device: ExtendedKalmanFilterBank with IteratedExtendedKalmanFilter's
    correct!, one (maxiters, epsilon) for the bank.  The lanes of a wave stop after different numbers of linearisations; a step costs
    what its slowest lane needs."""

    def __init__(self, filters_spec, device=0, Ts=1.0, maxiters=10, epsilon=1e-8):
        super().__init__(filters_spec, device, Ts)
        self.set_iterations(maxiters, epsilon)

    @classmethod
    def from_filter_bank(cls, bank, device=None, maxiters=10, epsilon=1e-8):
        """the iterated extended twin of a FilterBank (ExtendedKalmanFilterBank.from_filter_bank)"""
        self = super().from_filter_bank(bank, device)
        self.set_iterations(maxiters, epsilon)
        return self

    def set_iterations(self, maxiters, epsilon):
        """(maxiters, epsilon) of every later run (llpf_ekf_bank_set_iterations); (1, 0.0) is the extended filter"""
        self._h.set_iterations(maxiters, epsilon)
        self.maxiters, self.epsilon = int(maxiters), float(epsilon)


def _check_inflation(rho):
    rho = float(rho)
    if not np.isfinite(rho) or rho < 1.0:
        raise ValueError("enkf: the inflation must be finite and >= 1")
    return rho


class EnsembleKalmanFilter(_NonlinearKalmanFilter):
    """EnsembleKalmanFilter(dynamics, measurement, R1, R2, d0, N; inflation=1.0, Ts, nu, ny, p, seed, device) — the stochastic
    (perturbed-observation) ensemble Kalman filter with N members: every member is propagated through the dynamics with its own process
    noise, and one ny x ny solve from the ensemble's sample moments moves every member towards its own perturbed measurement
    (csrc/shared/llpf_enkf.h is the definition; unverified against the reference's EnsembleKalmanFilter).  The arguments are
    UnscentedKalmanFilter's, with two additions a ParticleFilter has: R1 may be a UserNoise and d0 a UserInitial when the UserDynamics
    snippet has a `noise` / `initial` member of its own (multiplicative or Laplace process noise, a box prior).  R2 stays Gaussian.
    state(f) is the ensemble mean, covariance(f) the sample covariance, particles(f) the members [N, nx].  Runs on the device as a bank of
    one filter (llpf_enkf_bank_*), created on first use.  nx <= 8, ny <= 4, nu <= 8, 2 <= N <= 65536."""

    def __init__(self, dynamics, measurement, R1, R2, d0, N, *, inflation=1.0, Ts=1.0, nu=-1, ny=-1, p=None, seed=0, device=0):
        if (isinstance(R1, UserNoise) or isinstance(d0, UserInitial)) and not isinstance(dynamics, UserDynamics):
            raise TypeError("UserNoise / UserInitial are members of a UserDynamics snippet")
        nx = dynamics.nx if isinstance(dynamics, UserDynamics) else len(d0)
        if ny < 0 and np.ndim(R2) >= 1:
            ny = np.asarray(R2).shape[0]
        if _is_plain_callable(dynamics):
            if ny < 0:
                raise ValueError("pass ny= with callable dynamics and a scalar R2")
            dynamics, measurement, _ = _trace_callables(dynamics, measurement, None, nx, nu, ny, p)
        if isinstance(dynamics, UserDynamics):
            ny = dynamics.ny
        elif isinstance(measurement, LinearMeasurement):
            ny = measurement.C.shape[0]
        elif isinstance(measurement, QuadTankMeasurement):
            ny = 2
        cov = lambda c, n: MvNormal(np.zeros(n), c if np.ndim(c) < 2 else np.atleast_2d(np.asarray(c, float)))
        self.dynamics, self.measurement, self.R1, self.R2, self.d0 = dynamics, measurement, R1, R2, d0
        self.dynamics_density = R1 if isinstance(R1, UserNoise) else cov(R1, nx)
        self.measurement_density, self.initial_density = cov(R2, ny), d0
        self.p, self.Ts, self.device = p, float(Ts), int(device)
        self._model = _build_model(dynamics, measurement, self.dynamics_density, self.measurement_density, d0, Ts)
        self.nx, self.nu, self.ny = self._model.nx, self._model.nu, self._model.ny
        self._handle = None
        self._index = 0
        self.N, self.seed, self.inflation = int(N), int(seed), _check_inflation(inflation)

    def _open(self):
        h = _capi.EnkfBankHandle(self.device, [self._model], self.N, self.seed)
        if self.inflation != 1.0:
            h.set_inflation(self.inflation)
        return h

    def set_inflation(self, rho):
        self.inflation = _check_inflation(rho)
        self._h.set_inflation(self.inflation)

    def members(self):
        """the members, [N, nx]"""
        return self._h.get_members()[0]


class EnsembleKalmanFilterBank(_KfBank):
    """n independent ensemble Kalman filters of N members each, of the same model family and dimensions, on one device, one GPU workgroup
    each (llpf_enkf_bank_*): a log-likelihood per parameter set without resampling, weights or ancestors, for every model a FilterBank
    takes except one with a likelihood of its own.  `filters_spec` is a list of EnsembleKalmanFilter or of (dynamics, measurement, R1, R2,
    d0) tuples; filter k's key is seed + k."""
    _AT_LOGLIK, _AT_FORWARD = {"t_index0": 1.0}, {"t_index0": 0.0}

    def __init__(self, filters_spec, N, device=0, seed=0, inflation=1.0, Ts=1.0):
        self._init(self._models(filters_spec, N, Ts), N, device, seed, inflation)

    def _init(self, models, N, device, seed, inflation):
        self.device, self.N, self.seed, self.inflation = int(device), int(N), int(seed), _check_inflation(inflation)
        self._h = _capi.EnkfBankHandle(self.device, models, self.N, self.seed)
        if self.inflation != 1.0:
            self._h.set_inflation(self.inflation)
        self.n_filters = len(models)
        self.Ts = float(models[0].Ts)

    @staticmethod
    def _models(filters_spec, N, Ts):
        return [(f if isinstance(f, EnsembleKalmanFilter) else EnsembleKalmanFilter(*f, N, Ts=Ts))._model for f in filters_spec]

    @classmethod
    def from_filter_bank(cls, bank, device=None, inflation=1.0):
        """the ensemble twin of a FilterBank: the same descriptors (any model that is not Rao-Blackwellized and has no likelihood of its
        own), N members where the bank has N particles, the bank's seed; loglik and forward at the times FilterBank's use"""
        self = cls.__new__(cls)
        self._init(list(bank._models), bank.N, bank._h.cfg.device if device is None else device, bank.rng, inflation)
        return self

    def set_parameters(self, filters_spec):
        """new parameters for every filter (same model and dimensions, nothing reallocated: llpf_enkf_bank_set_models)"""
        self._h.set_models(self._models(filters_spec, self.N, self.Ts))

    def set_inflation(self, rho):
        self.inflation = _check_inflation(rho)
        self._h.set_inflation(self.inflation)

    def members(self):
        """the members of every filter, [F, N, nx]"""
        return self._h.get_members()

    def smooth(self, u, y, outputs=None, forward=()):
        raise TypeError("the ensemble Kalman filter has no smoother")


class RBMeasurementModel:
    """RBMeasurementModel(measurement, R2, ny) — reference src/rbpf.jl:36-60; `measurement` is a LinearMeasurement
    descriptor of the nonlinear state's contribution y = Gn xn (+ C xl + e)."""

    def __init__(self, measurement, R2, ny):
        self.measurement, self.R2, self.ny = measurement, R2, int(ny)


class StateAffineCoupling:
    """An as a function of the state (reference src/rbpf.jl:108: "`An` may be a matrix or a function of x, u, p, t that
    returns a matrix"), in the descriptor form the GPU can run: An(xn) = An0 + sum_k xn[k] Ank[k]."""

    def __init__(self, An0, Ank):
        self.An0 = np.atleast_2d(np.asarray(An0, dtype=np.float64))
        self.Ank = np.asarray(Ank, dtype=np.float64).reshape((self.An0.shape[0],) + self.An0.shape)

    def __call__(self, x, u=None, p=None, t=0.0):
        xn = np.asarray(getattr(x, "xn", x), dtype=np.float64)[: self.An0.shape[0]]
        return self.An0 + np.tensordot(xn, self.Ank, axes=(0, 0))


class RBPF(_AbstractParticleFilter):
    """RBPF(N, kf, dynamics, nl_measurement_model, R1n, d0n; An, nu, Ts, rng, resample_threshold) — the
    Rao-Blackwellized ("marginalized") particle filter of reference src/rbpf.jl:63-144.  With constant matrices
    (dynamics = LinearDynamics(Fn, Bn) of the nonlinear substate, An a matrix or None) one covariance serves all
    particles; with An = StateAffineCoupling(...) every particle carries its own Kalman filter (the reference's
    !singleR branches, :176/:247), and dynamics / nl_measurement_model.measurement may also be the quad-tank
    descriptors."""
    kind = S.PARTICLE_FILTER

    def __init__(self, N, kf, dynamics, nl_measurement_model, R1n, d0n, *, An=None, nu=-1, Ts=1.0, p=None, rng=None,
                 resample_threshold=0.1, names=None, device=0):
        if isinstance(kf, SqKalmanFilter):
            raise TypeError("RBPF: the inner filter is a KalmanFilter; a SqKalmanFilter is not supported")
        if np.any(np.asarray(0.0 if kf.D is None else kf.D) != 0):
            raise NotImplementedError("D != 0")
        as_g = lambda d: d.struct() if isinstance(d, MvNormal) else d
        as_cov = lambda d, n: d if not isinstance(d, (np.ndarray, list)) else MvNormal(np.zeros(n), np.atleast_2d(np.asarray(d, float)))
        nn = 4 if isinstance(dynamics, QuadTankDynamics) else np.atleast_2d(np.asarray(dynamics.A, float)).shape[0]
        R1n = as_cov(R1n, nn)
        R2 = as_cov(nl_measurement_model.R2, nl_measurement_model.ny)
        mm = nl_measurement_model.measurement
        Gn = np.zeros((nl_measurement_model.ny, nn)) if mm is None else getattr(mm, "C", None)
        self.kf, self.dynamics, self.nl_measurement_model, self.An, self.R1n, self.d0n = kf, dynamics, nl_measurement_model, An, R1n, d0n
        self.resample_threshold = float(resample_threshold)
        self.resampling_strategy = ResampleSystematic            # resampling_strategy(pf::RBPF), src/rbpf.jl:306
        self.rng = 0 if rng is None else int(rng)
        self.p, self.Ts, self.names, self.threads = p, float(Ts), names, False
        self.measurement_likelihood = None
        self.per_particle_covariance = isinstance(An, StateAffineCoupling)
        if self.per_particle_covariance:
            Ast = np.concatenate([An.An0[None], An.Ank], axis=0)
            if isinstance(dynamics, QuadTankDynamics):
                self._model = S.make_rb_bilinear_model(Ast, kf.A, kf.B, kf.C, as_g(R1n), kf.R1, as_g(R2), as_g(d0n), as_g(kf.d0),
                                                       quadtank=dynamics.consts, Ts=Ts, supersample=dynamics.supersample)
            else:
                self._model = S.make_rb_bilinear_model(Ast, kf.A, kf.B, kf.C, as_g(R1n), kf.R1, as_g(R2), as_g(d0n), as_g(kf.d0),
                                                       Fn=dynamics.A, Bn=dynamics.B, Gn=Gn, Ts=Ts)
        else:
            self._model = S.make_rb_model(dynamics.A, dynamics.B, An, kf.A, kf.B, Gn, kf.C, as_g(R1n), kf.R1, as_g(R2), as_g(d0n), as_g(kf.d0), Ts)
        self.nx, self.nu, self.ny = self._model.nx, self._model.nu, self._model.ny
        if self.per_particle_covariance:
            self.nx = self._model.nx + self._model.rb.nxl      # particles are [xn; xl]
        self._cfg = S.make_config(self._model, N, self.kind, S.RESAMPLE_SYSTEMATIC, resample_threshold, self.rng, device)
        self._h = _capi.FilterHandle(self._cfg)
        self.N = int(N)

    @property
    def covariance(self):
        """x[1].R: the covariance of the linear substate (shared by all particles for constant matrices)."""
        if self.per_particle_covariance:
            return self._h.rb_linear_state()[1][0]
        return self._h.rb_covariance()

    def linear_state(self):
        """(xl [N, nxl], R [N, nxl, nxl]): the fields xl, R of every RBParticle (reference src/rbpf.jl:1-5)."""
        if not self.per_particle_covariance:
            nn = self._model.nxn
            xl = self._h.particles()[:, nn:]
            return xl, np.broadcast_to(self._h.rb_covariance(), (self.N,) + self._h.rb_covariance().shape).copy()
        return self._h.rb_linear_state()


class AuxiliaryParticleFilter:
    """AuxiliaryParticleFilter(args...; kwargs...) = AuxiliaryParticleFilter(ParticleFilter(args...; kwargs...)) or
    AuxiliaryParticleFilter(pf) — reference src/PFtypes.jl:38-49.  Everything but predict!/correct!/update!/
    forward_trajectory/loglik is forwarded to the wrapped filter (PFtypes.jl:101-105, 299)."""

    def __init__(self, *args, **kwargs):
        if len(args) == 1 and not kwargs and isinstance(args[0], _AbstractParticleFilter):
            pf = args[0]
        else:
            pf = ParticleFilter(*args, **kwargs)
        object.__setattr__(self, "pf", pf)

    def __getattr__(self, name):            # getproperty forwarding, src/PFtypes.jl:101-105
        return getattr(object.__getattribute__(self, "pf"), name)

    # pf(u, y, y1, p, t): update! (reference src/filtering.jl:239)
    def __call__(self, u, y, y1, p=None, t=None):
        return update(self, u, y, y1, p, t)


class _StateView:
    """Read-only view with the reference's PFstate field names (src/PFtypes.jl:8-17)."""

    def __init__(self, pf):
        self._pf = pf

    x = property(lambda s: s._pf._h.particles())
    xprev = property(lambda s: s._pf._h.particles())    # xprev == x outside predict! (copyto!, filtering.jl:151)
    w = property(lambda s: s._pf._h.weights())
    we = property(lambda s: s._pf._h.expweights())
    maxw = property(lambda s: s._pf._h.maxw())
    j = property(lambda s: s._pf._h.ancestors())
    bins = property(lambda s: s._pf._h.bins())
    t = property(lambda s: s._pf._h.index())


class ParticleFilteringSolution:
    """Fields f,u,y,x,w,we,ll,t of the reference's struct (src/solutions.jl:334-345).  x is [T, N, nx]
    (column t of the reference's N x T matrix of SVectors is x[t]); w, we are [T, N]."""

    def __init__(self, f, u, y, x, w, we, ll, quantile_p=None, xquant=None):
        self.f, self.u, self.y, self.x, self.w, self.we, self.ll = f, u, y, x, w, we, ll
        self.t = np.arange(x.shape[0]) * f.Ts
        # forward_trajectory(..., quantiles=q): weighted_quantile of every timestep, computed on the device inside the run loop
        self.quantile_p = None if quantile_p is None else np.atleast_1d(np.asarray(quantile_p, dtype=np.float64))
        self.xquant = xquant                      # [T, nx, len(quantile_p)]


# ---------------------------------------------------------------------------------------------------
# verbs
# ---------------------------------------------------------------------------------------------------
def reset(pf):
    """reset!(pf) — reference src/filtering.jl:4-14 (src/kalman.jl:159-164 for a KalmanFilter)."""
    if isinstance(pf, (_NonlinearKalmanFilter, IMM)):
        return pf.reset()
    pf._h.reset()


def _t(pf, t):
    return pf._h.index() * pf.Ts if t is None else float(t)


def _pt(args, kw, skip):
    """(p, t) from the trailing positional / keyword arguments of a verb."""
    rest = list(args[skip:])
    p = rest[0] if len(rest) > 0 else kw.get("p")
    t = rest[1] if len(rest) > 1 else kw.get("t")
    return p, t


def predict(pf, u, *args, **kw):
    """predict!(pf, u, p, t = index(pf)*Ts) — reference src/filtering.jl:140-153;
    predict!(pf::AuxiliaryParticleFilter, u, y1, p, t) — :195-217 (y1 = the NEXT measurement)."""
    if isinstance(pf, EnsembleKalmanFilter):        # the bank's own verb: the members move, the step counter grows
        t = _pt(args, kw, 0)[1]
        pf._h.predict(u, t_index=float(pf._index) if t is None else float(t) / pf.Ts)
        pf._index += 1
        return
    if isinstance(pf, _NonlinearKalmanFilter):      # a step whose measurement is missing: correct! is skipped, predict! runs
        pf._step(u, None, _pt(args, kw, 0)[1], ())
        return
    if isinstance(pf, AuxiliaryParticleFilter):
        y1 = args[0] if args else kw.get("y1")
        pf._h.aux_predict(u, y1, _t(pf, _pt(args, kw, 1)[1]))
        return
    pf._h.predict(u, _t(pf, _pt(args, kw, 0)[1]))


def correct(pf, u, y, p=None, t=None):
    """ll, 0 = correct!(pf, u, y, p, t) — reference src/filtering.jl:164-168.  y=None means missing.
    For an AuxiliaryParticleFilter (:170-174) only logsumexp! runs: the measurement update was done in predict!."""
    if isinstance(pf, EnsembleKalmanFilter):
        if y is None:
            return 0.0, np.full(pf.ny, np.nan)
        ll, e = pf._h.correct(u, y, t_index=float(pf._index) if t is None else float(t) / pf.Ts)
        return float(ll[0]), e[0]
    if isinstance(pf, _NonlinearKalmanFilter):
        # the posterior of a one-step run put back as the state: the same numbers (the packed lower triangle of Rt is what the step holds)
        i = pf._index
        r = pf._step(u, y, t, ("xt", "Rt", "e"))
        pf._h.set_state(r["xt"][0], r["Rt"][0])
        pf._index = i
        return float(r["ll"][0]), r["e"][0, 0]
    if isinstance(pf, AuxiliaryParticleFilter):
        return pf._h.aux_correct(), 0
    return pf._h.correct(u, y, _t(pf, t)), 0


def update(pf, u, y, *args, **kw):
    """ll, 0 = update!(pf, u, y, p, t) — reference src/filtering.jl:181-185;
    update!(pf::AuxiliaryParticleFilter, u, y, y1, p, t) — :187-191.
    ll, e = update!(kf::KalmanFilter, u, y): correct! then predict!, continuing the filter's state."""
    if isinstance(pf, KalmanFilter):
        r = pf._run(np.atleast_1d(np.asarray(0.0 if u is None else u, float))[None], np.atleast_1d(np.asarray(y, float))[None], ("e",))
        return float(r["ll"][0]), r["e"][0, 0]
    if isinstance(pf, IMM):                         # the step of csrc/shared/llpf_imm.h; an IMM has no single innovation
        t = _pt(args, kw, 0)[1]                     # (extended, unscented modes: the step's time, default index * Ts as the nonlinear filters')
        r = pf._run(np.atleast_1d(np.asarray(0.0 if u is None else u, float))[None], np.atleast_1d(np.asarray(y, float))[None], (),
                    float(pf._index) if t is None else float(t) / pf.Ts)
        return float(r["ll"][0]), None
    if isinstance(pf, _NonlinearKalmanFilter):
        r = pf._step(u, y, _pt(args, kw, 0)[1], ("e",))
        return float(r["ll"][0]), r["e"][0, 0]
    if isinstance(pf, AuxiliaryParticleFilter):
        y1 = args[0] if args else kw.get("y1")
        return pf._h.aux_update(u, y1, _t(pf, _pt(args, kw, 1)[1])), 0
    return pf._h.update(u, y, _t(pf, _pt(args, kw, 0)[1])), 0


def forward_trajectory(pf, u, y, p=None, quantiles=None):
    """sol = forward_trajectory(pf, u, y, p) — reference src/filtering.jl:343-365 (:367-384 for the auxiliary
    filter).  The whole T-step loop is enqueued on the device; callbacks of the reference signature are not
    supported (a fused on-device loop cannot call back into the host) — drive update() step by step if needed.
    quantiles=q (not for the auxiliary filter): weighted_quantile(sol, q) of every timestep is computed on the device inside the run loop
    (llpf_run's xquant output) and kept in the solution; weighted_quantile(sol, q') with q' among q is then served from it.
    For a KalmanFilter: the reference's KalmanFilteringSolution (src/filtering.jl forward_trajectory), computed on the device."""
    if isinstance(pf, KalmanFilter):
        reset(pf)
        r = pf._run(u, y, _capi.KALMAN_OUTPUTS)
        return KalmanFilteringSolution(pf, u, y, r["x"][:, 0], r["xt"][:, 0], r["R"][:, 0], r["Rt"][:, 0], float(r["ll"][0]), r["e"][:, 0])
    if isinstance(pf, IMM):
        reset(pf)
        r = pf._run(u, y, _capi.IMM_OUTPUTS)
        return IMMFilteringSolution(pf, u, y, r["x"][:, 0], r["xt"][:, 0], r["R"][:, 0], r["Rt"][:, 0], float(r["ll"][0]), r["mu"][:, 0],
                                    r["ll_modes"][:, 0])
    if isinstance(pf, _NonlinearKalmanFilter):
        reset(pf)
        r = pf._run(u, y, _capi.KALMAN_OUTPUTS, 0.0)
        return KalmanFilteringSolution(pf, u, y, r["x"][:, 0], r["xt"][:, 0], r["R"][:, 0], r["Rt"][:, 0], float(r["ll"][0]), r["e"][:, 0])
    reset(pf)
    if isinstance(pf, AuxiliaryParticleFilter):
        if quantiles is not None:
            raise ValueError("forward_trajectory(quantiles=...) is not provided for the auxiliary filter: use weighted_quantile(sol, q)")
        r = pf._h.run_aux(u, y, mode=0, history=True)
    else:
        r = pf._h.run(u, y, t_index0=0.0, history=True, quantiles=quantiles)
    return ParticleFilteringSolution(pf, u, y, r["x"], r["w"], r["we"], r["ll"], quantiles, r.get("xquant"))


def loglik(pf, u, y, p=None):
    """loglik(pf, u, y, p) — reference src/smoothing.jl:227-230 (reset!, then sum of update! with
    t = index(pf)*Ts, i.e. the first step is at t = 1*Ts); :232-236 for the auxiliary filter (t = (k-1)*Ts, the
    last step is an update! of the wrapped filter).  For a KalmanFilter: reset!, then the sum of T update! steps (exact)."""
    reset(pf)
    if isinstance(pf, IMM):                         # extended, unscented modes: the first step at t = 1 * Ts, as those filters' loglik
        return float(pf._run(u, y, (), 1.0 if pf._timed else 0.0)["ll"][0])
    if isinstance(pf, KalmanFilter):
        return float(pf._run(u, y)["ll"][0])
    if isinstance(pf, _NonlinearKalmanFilter):      # the first step at t = 1 * Ts, as the particle filters' loglik
        return float(pf._run(u, y, (), 1.0)["ll"][0])
    if isinstance(pf, AuxiliaryParticleFilter):
        return pf._h.run_aux(u, y, mode=1)["ll"]
    return pf._h.run(u, y, t_index0=1.0)["ll"]


def log_likelihood_fun(filter_from_parameters, priors, u, y):
    """ll = log_likelihood_fun(filter_from_parameters, priors, u, y) — reference src/smoothing.jl:266-283: theta -> log prior + loglik of
    the filter built from theta; -inf outside the priors' support or when the filter degenerates.  `filter_from_parameters(theta, pf)` is
    called with the previous filter (None the first time) so that it can return `pf.set_parameters(...)` instead of a new filter;
    a function of theta alone is accepted too.  `priors[i]` is anything with a `logpdf(x)` method (scipy.stats frozen distributions)."""
    import inspect
    try:
        two = len(inspect.signature(filter_from_parameters).parameters) >= 2
    except (TypeError, ValueError):
        two = False
    state = {"pf": None}

    def ll(theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.size != len(priors):
            raise ValueError("Input must have same length as priors")
        lp = float(sum(np.float64(priors[i].logpdf(theta[i])) for i in range(theta.size)))
        if not np.isfinite(lp):
            return -np.inf
        state["pf"] = filter_from_parameters(theta, state["pf"]) if two else filter_from_parameters(theta)
        try:
            return lp + loglik(state["pf"], u, y)
        except (_capi.LLPFError, ValueError, FloatingPointError):
            return -np.inf
    return ll


def naive_sampler(theta0, rng=None):
    """theta -> theta + N(0, diag(0.1 |theta0|)) — reference src/smoothing.jl:284-287"""
    theta0 = np.asarray(theta0, dtype=np.float64)
    if np.any(theta0 == 0):
        raise ValueError("Naive sampler does not work if initial parameter vector contains zeros")
    rng = np.random.default_rng() if rng is None else rng
    sd = np.sqrt(0.1 * np.abs(theta0))
    return lambda theta: np.asarray(theta) + sd * rng.standard_normal(theta0.size)


def metropolis(ll, R, theta0, draw=None, rng=None):
    """params, lls = metropolis(ll, R, theta0, draw) — reference src/smoothing.jl:311-330: marginal Metropolis with a symmetric proposal;
    `rng` (numpy Generator) supplies the acceptance uniforms (the reference uses the global rand())."""
    rng = np.random.default_rng() if rng is None else rng
    draw = naive_sampler(theta0, rng) if draw is None else draw
    params, lls = [np.asarray(theta0, dtype=np.float64)], [float(ll(theta0))]
    for _ in range(1, int(R)):
        theta = np.asarray(draw(params[-1]), dtype=np.float64)
        lli = float(ll(theta))
        if rng.random() < np.exp(lli - lls[-1]):
            params.append(theta); lls.append(lli)
        else:
            params.append(params[-1]); lls.append(lls[-1])
    return params, np.array(lls)


def _build_spec(spec_from_parameters, theta, Ts):
    """the llpf_model of a candidate; ValueError / TypeError / LinAlgError if the library would not accept it (densities positive definite,
    dimensions as declared).  A model's own densities (UserNoise, UserInitial) carry no covariance: the Gaussian that stands in for them
    in the descriptor is checked where one was given (UserNoise.gaussian)."""
    dy, me, df, dg, d0 = spec_from_parameters(theta)
    model = _build_model(dy, me, df, dg, d0, Ts)
    for d in (df.gaussian if isinstance(df, UserNoise) else df, dg, None if isinstance(d0, UserInitial) else d0):
        if d is None:
            continue
        c = np.asarray(d.cov, dtype=np.float64)      # what the library's gauss_prepare (csrc/host/densities.hpp:23) asks of a covariance
        if not np.all(np.isfinite(c)) or not np.all(np.diag(c) > 0.0):
            raise ValueError("covariance not finite or not positive")
        np.linalg.cholesky(c)
    return model


def _spec_builds(spec_from_parameters, theta, Ts=1.0):
    """the model of this candidate, or None if it is one the library would refuse.  Only what a bad PARAMETER VALUE raises is caught: an error
    of the caller's spec_from_parameters itself (AttributeError, KeyError, ...) is a bug to be seen, not a rejected proposal."""
    try:
        return _build_spec(spec_from_parameters, theta, Ts)
    except (ValueError, TypeError, np.linalg.LinAlgError):
        return None


def metropolis_bank(bank, spec_from_parameters, priors, u, y, R, theta0s, draw=None, burnin=0, rng=None):
    """The GPU form of the reference's metropolis_threaded (src/smoothing.jl:335-347: one independent chain per thread): the chains advance in
    lockstep and every iteration is ONE bank run — llpf_bank_set_models with the chains' candidates, then the bank's loglik.
    `bank`: a FilterBank with one filter per chain; `spec_from_parameters(theta)` -> (dynamics, measurement, df, dg, d0) of a candidate;
    `theta0s`: [n_chains, n_parameters].  Returns an array [(R - burnin) * n_chains, n_parameters + 1], log-likelihoods (with the log
    prior) in the last column, chain after chain — the layout metropolis_threaded returns."""
    rng = np.random.default_rng() if rng is None else rng
    theta0s = np.atleast_2d(np.asarray(theta0s, dtype=np.float64))
    n = theta0s.shape[0]
    if n != bank.n_filters:
        raise ValueError("one chain per filter of the bank")
    draw = (lambda th, d=naive_sampler(theta0s[0], rng): d(th)) if draw is None else draw

    import re

    def lls_of(thetas, prebuilt=None):
        lp = np.array([sum(np.float64(priors[i].logpdf(th[i])) for i in range(th.size)) for th in thetas])
        ok = np.isfinite(lp)
        # Chains whose candidate lies outside the priors' support keep a valid model in their slot; its likelihood is not used.  A chain
        # whose candidate cannot be built (covariance not positive definite) or degenerates the filter scores -inf ALONE — the reference
        # wraps each chain's loglik in try / catch (src/smoothing.jl:276-280), so one bad proposal must not stop the others: the failing
        # slot (the library's message names the filter) is given its chain's current parameters and the bank runs again.
        # Candidates that cannot be BUILT are found on the host first (cheap: no device work), all of them at once — what can still cost a
        # rerun is a filter that degenerates on the device or a density that only the library refuses (a variance that underflowed to
        # zero passes the host's shape checks); the library names the first such filter.  An error that names no filter (bad shapes of
        # u / y, a lost device) is nobody's candidate and propagates at once.
        built = list(cur_models)
        for k in range(n):
            if ok[k]:
                m = prebuilt[k] if prebuilt is not None else _spec_builds(spec_from_parameters, thetas[k], bank.Ts)
                if m is None:
                    ok[k] = False
                else:
                    built[k] = m
        ll = None
        for _ in range(n + 1):
            try:
                bank.set_models([built[k] if ok[k] else cur_models[k] for k in range(n)])      # the models built above, not built again
                ll = bank.loglik(u, y)
                break
            except _capi.LLPFError as e:                 # DegenerateWeights is one
                m = re.search(r"in filter (\d+)", str(e))
                bad = int(m.group(1)) if m else None
                if bad is None or not ok[bad]:
                    raise
                ok[bad] = False
        if ll is None:
            raise RuntimeError("metropolis_bank: the bank fails with every chain on its current parameters")
        out = np.where(ok, lp + ll, -np.inf)
        return np.where(np.isnan(out), -np.inf, out), built

    # The starting parameters have nothing to fall back on: one that cannot be built is an error of the call (and says why), not a chain
    # that scores -inf for ever.
    cur = theta0s.copy()
    cur_models = []
    for k in range(n):
        try:
            cur_models.append(_build_spec(spec_from_parameters, cur[k], bank.Ts))
        except (ValueError, TypeError, np.linalg.LinAlgError) as e:
            raise ValueError("metropolis_bank: the starting parameters of chain %d cannot be built: %s" % (k, e)) from e
    ll_cur, _ = lls_of(cur, cur_models)
    chain = np.empty((int(R), n, theta0s.shape[1] + 1))
    chain[0, :, :-1], chain[0, :, -1] = cur, ll_cur
    for i in range(1, int(R)):
        cand = np.stack([np.asarray(draw(cur[k]), dtype=np.float64) for k in range(n)])
        ll_c, built = lls_of(cand)
        acc = rng.random(n) < np.exp(ll_c - ll_cur)
        cur = np.where(acc[:, None], cand, cur)
        cur_models = [built[k] if acc[k] else cur_models[k] for k in range(n)]
        ll_cur = np.where(acc, ll_c, ll_cur)
        chain[i, :, :-1], chain[i, :, -1] = cur, ll_cur
    return np.concatenate([chain[int(burnin):, k, :] for k in range(n)], axis=0)


def weighted_cov(x, we=None):
    """weighted_cov(x, we) / weighted_cov(sol) — reference src/filtering.jl:573-581: per time step the covariance of
    the particles under probability weights with StatsBase's correction n / ((n - 1) sum(w)), n = count(w != 0).
    weighted_cov(pf): the current particles and weights of a filter, computed on the device (llpf_weighted_cov)."""
    if isinstance(x, _AbstractParticleFilter):
        return x._h.weighted_cov()
    if isinstance(x, ParticleFilteringSolution):
        x, we = x.x, x.we
    x, we = np.asarray(x), np.asarray(we)
    out = []
    for t in range(x.shape[0]):
        w = we[t]
        s = w.sum()
        mu = (x[t] * w[:, None]).sum(axis=0) / s
        d = x[t] - mu
        n = np.count_nonzero(w)
        out.append((d * w[:, None]).T @ d * (n / ((n - 1) * s)))
    return out


def _statsbase_quantile(v, w, q):
    """StatsBase.quantile(v, ProbabilityWeights(w), q) (src/weights.jl, the branch for non-frequency weights), vectorised over q"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.isnan(v).any():
        return np.full(q.shape, np.nan)
    keep = w != 0
    order = np.lexsort((w[keep], v[keep]))           # tuples (v, w) sort lexicographically
    vs, ws = v[keep][order], w[keep][order]
    S = np.cumsum(ws)
    h = q * (w.sum() - ws[0]) + ws[0]
    k = np.searchsorted(S, h, side="right")          # first k with S_k > h
    past = k >= vs.size
    k = np.minimum(k, vs.size - 1)
    Skold = np.where(k > 0, S[np.maximum(k - 1, 0)], 0.0)
    vkold = np.where(k > 0, vs[np.maximum(k - 1, 0)], 0.0)
    return np.where(past, vs[-1], vkold + (h - Skold) / (S[k] - Skold) * (vs[k] - vkold))


def weighted_quantile(x, we=None, q=None):
    """weighted_quantile(x, we, q) / weighted_quantile(sol, q) — reference src/filtering.jl:583-595: per time step and state dimension the
    weighted quantile of the particles (StatsBase's definition), a list of length T of [nx, len(q)] arrays (of nx-vectors for a scalar q):
    the reference's nesting [t][state][q].
    weighted_quantile(pf, q): the current particles and weights of a filter, sorted and summed on the device (llpf_weighted_quantile);
    [nx, len(q)] like one time step of the above (the C ABI itself writes [nq][nx]; the Julia accessor returns nx x nq as well)."""
    if isinstance(x, _AbstractParticleFilter):
        qq = we if q is None else q
        out = x._h.weighted_quantile(qq)
        return out[0] if np.isscalar(qq) else np.ascontiguousarray(out.T)
    if isinstance(x, ParticleFilteringSolution):
        sol, q = x, (we if q is None else q)
        if sol.xquant is not None:       # computed by the run loop on the device: served from there when every q was asked for
            qq = np.atleast_1d(np.asarray(q, dtype=np.float64))
            idx = [np.flatnonzero(sol.quantile_p == v) for v in qq]
            if all(len(i) for i in idx):
                sel = sol.xquant[:, :, [int(i[0]) for i in idx]]
                return [sel[t][:, 0].copy() if np.isscalar(q) else sel[t].copy() for t in range(sel.shape[0])]
        x, we = sol.x, sol.we
    x, we = np.asarray(x), np.asarray(we)
    out = []
    for t in range(x.shape[0]):
        r = np.stack([_statsbase_quantile(x[t][:, d], we[t], q) for d in range(x.shape[2])], axis=0)      # [state][q]
        out.append(r[:, 0] if np.isscalar(q) else r)
    return out


def mode_trajectory(x, we=None):
    """mode_trajectory(sol) / (x, we) — reference src/filtering.jl:415,436: the particle with the largest weight, T x nx."""
    if isinstance(x, ParticleFilteringSolution):
        x, we = x.x, x.we
    x, we = np.asarray(x), np.asarray(we)
    return x[np.arange(x.shape[0]), np.argmax(we, axis=1)]


def smooth(pf, *args):
    """xb, ll = smooth(pf, M, u, y, p) / smooth(pf, xf, wf, wef, ll, M, u, y, p) — forward filtering, backward
    simulation (reference src/smoothing.jl:103-143).  xb is [T, M, nx].
    sol = smooth(kf::KalmanFilter, u, y, p) — reset!, forward_trajectory and the Rauch-Tung-Striebel smoother (src/smoothing.jl:10-102),
    on the device: a KalmanSmoothingSolution.
    sol = smooth(ukf::UnscentedKalmanFilter, u, y, p) — reset!, forward_trajectory and the unscented Rauch-Tung-Striebel smoother
    (csrc/shared/llpf_ukf.h: llpf_ukf_smooth_finish), on the device: a KalmanSmoothingSolution."""
    if isinstance(pf, SqKalmanFilter):
        raise TypeError("the square-root Kalman filter has no smoother")
    if isinstance(pf, SqExtendedKalmanFilter):
        raise TypeError("the square-root extended Kalman filter has no smoother")
    if isinstance(pf, AugmentedUnscentedKalmanFilter):
        raise TypeError("the augmented unscented Kalman filter has no smoother")
    if isinstance(pf, KalmanFilter):
        u, y = args[:2]
        reset(pf)
        yy = np.asarray(y, dtype=np.float64)
        yy = yy.reshape(yy.shape[0], -1) if yy.ndim else yy.reshape(1, 1)
        uu = None if pf._h.nu == 0 else np.asarray(u, dtype=np.float64).reshape(yy.shape[0], -1)
        r = pf._h.smooth(uu, yy, forward=_capi.KALMAN_OUTPUTS)
        sol = KalmanFilteringSolution(pf, u, y, r["x"][:, 0], r["xt"][:, 0], r["R"][:, 0], r["Rt"][:, 0], float(r["ll"][0]), r["e"][:, 0])
        return KalmanSmoothingSolution(sol, r["xT"][:, 0], r["RT"][:, 0])
    if isinstance(pf, UnscentedKalmanFilter):      # the first step at t = 0, as forward_trajectory counts time
        u, y = args[:2]
        reset(pf)
        yy = np.asarray(y, dtype=np.float64)
        yy = yy.reshape(yy.shape[0], -1) if yy.ndim else yy.reshape(1, 1)
        uu = None if pf.nu == 0 else np.asarray(u, dtype=np.float64).reshape(yy.shape[0], -1)
        r = pf._h.smooth(uu, yy, forward=_capi.KALMAN_OUTPUTS, t_index0=0.0)
        pf._index += yy.shape[0]
        sol = KalmanFilteringSolution(pf, u, y, r["x"][:, 0], r["xt"][:, 0], r["R"][:, 0], r["Rt"][:, 0], float(r["ll"][0]), r["e"][:, 0])
        return KalmanSmoothingSolution(sol, r["xT"][:, 0], r["RT"][:, 0])
    if isinstance(pf, IMM):
        raise TypeError("the IMM filter has no smoother")
    if isinstance(pf, EnsembleKalmanFilter):
        raise TypeError("the ensemble Kalman filter has no smoother")
    if isinstance(pf, ExtendedKalmanFilter):
        raise TypeError("the extended Kalman filter has no smoother yet: smooth an UnscentedKalmanFilter of the same model")
    if isinstance(getattr(pf, "dynamics_density", None), UserNoise):      # before the forward pass: llpf_smooth would refuse after it
        raise TypeError("smooth is not defined for a model with process noise of its own (UserNoise): the backward weights are "
                        "logpdf(dynamics_density, .), and the model's transition density is not that Gaussian")
    if len(args) >= 7:
        xf, wf, wef, ll, M, u, y = args[:7]
    else:
        M, u, y = args[:3]
        sol = forward_trajectory(pf, u, y)
        xf, wf, wef, ll = sol.x, sol.w, sol.we, sol.ll
    xb, _ = pf._h.smooth(M, u, xf, wf, wef)
    return xb, ll


def smoothed_mean(xb):
    """smoothed_mean(xb) — reference src/smoothing.jl:356-361; returns [nx, T] like the reference's hcat."""
    return np.asarray(xb).mean(axis=1).T


def smoothed_cov(xb):
    """smoothed_cov(xb) — reference src/smoothing.jl:368-372: list of T covariance matrices (normalised by M-1)."""
    xb = np.asarray(xb)
    return [np.atleast_2d(np.cov(xb[t].T)) for t in range(xb.shape[0])]


def smoothed_trajs(xb):
    """smoothed_trajs(xb) — reference src/smoothing.jl:379-383: array (nx, M, T)."""
    return np.ascontiguousarray(np.transpose(np.asarray(xb), (2, 1, 0)))


def mean_trajectory(pf, u=None, y=None, p=None):
    """x̂, ll = mean_trajectory(pf, u, y) — reference src/filtering.jl:393, 417-432 (including its quirk:
    correct!(u[1], y[1], t=0) is followed by pf(u[t-1], y[t]) for t = 2..T).
    mean_trajectory(sol) — reference :405: T x nx matrix of weighted means."""
    if isinstance(pf, ParticleFilteringSolution):
        return np.einsum("tnd,tn->td", pf.x, pf.we)
    reset(pf)
    Y = np.asarray(y, dtype=np.float64).reshape(-1, pf.ny)
    Um = np.asarray(u, dtype=np.float64).reshape(Y.shape[0], -1)
    T = Y.shape[0]
    xh = np.zeros((T, pf.nx))
    ll = pf._h.correct(Um[0], Y[0], 0.0)
    xh[0] = pf._h.weighted_mean()
    for t in range(1, T):
        ll += pf._h.update(Um[t - 1], Y[t], t * pf.Ts)
        xh[t] = pf._h.weighted_mean()
    return xh, ll


# accessors — reference src/PFtypes.jl:296-334
def particles(pf):
    if isinstance(pf, EnsembleKalmanFilter):
        return pf.members()
    return pf._h.particles()


def weights(pf):
    return pf._h.weights()


def expweights(pf):
    return pf._h.expweights()


def state(pf):
    if isinstance(pf, (KalmanFilter, _NonlinearKalmanFilter, IMM)):
        return pf.x
    return pf.state


def num_particles(pf):
    return pf.N


def index(pf):
    return pf._h.index()


def parameters(pf):
    return pf.p


def dynamics(pf):
    return pf.dynamics


def measurement(pf):
    return pf.measurement


def measurement_likelihood(pf):
    return pf.measurement_likelihood


def dynamics_density(pf):
    return pf.dynamics_density


def measurement_density(pf):
    return pf.measurement_density


def initial_density(pf):
    return pf.initial_density


def resample_threshold(pf):
    return pf.resample_threshold


def resampling_strategy(pf):
    return pf.resampling_strategy


def effective_particles(pf_or_we):
    """effective_particles(pf | we) — reference src/resample.jl:1-2."""
    if isinstance(pf_or_we, _AbstractParticleFilter):
        return pf_or_we._h.ess()
    we = np.asarray(pf_or_we, dtype=np.float64)
    # ESS of a plain vector goes through the same normalise kernel: we are exp-weights => log them
    h = _weights_handle(we)
    return h.ess()


def _weights_handle(we):
    """A scratch 1-D filter holding log(we) as its weights (weights-only operations on plain vectors)."""
    g = MvNormal(np.zeros(1), 1.0)
    m = S.make_lg_model(np.eye(1), None, np.eye(1), g.struct(), g.struct(), g.struct())
    cfg = S.make_config(m, we.size)
    h = _capi.FilterHandle(cfg)
    with np.errstate(divide="ignore"):
        h.set_weights(np.log(we))
    return h


def shouldresample(pf):
    """shouldresample(pf) — reference src/resample.jl:5-10."""
    return pf._h.shouldresample()


def resample(a, we=None, M=None, U=None, seed=0, step=0):
    """resample(pf) / resample(T, we[, M]) / resample(we) — reference src/resample.jl:12-15.  Returns 0-based
    ancestor indices.  The uniforms the reference draws from the global RNG come from Philox(seed, step)
    unless given explicitly in U."""
    if isinstance(a, _AbstractParticleFilter):
        strategy, wev = a.resampling_strategy, a._h.expweights()
    elif we is None:
        strategy, wev = ResampleSystematic, np.asarray(a, dtype=np.float64)
    else:
        strategy, wev = a, np.asarray(we, dtype=np.float64)
    M = wev.size if M is None else int(M)
    if U is None:
        U = _capi.resample_uniforms(strategy.code, M, seed, step)
    return _capi.resample(strategy.code, wev, U, M)


def weighted_mean(pf):
    """weighted_mean(pf) — reference src/filtering.jl:541-549,568."""
    return pf._h.weighted_mean()


def logsumexp(w):
    """ll, w, we = logsumexp!(w, we) — reference src/utils.jl:18-27 (returns the normalised copies)."""
    return _capi.logsumexp(w)


def simulate(pf, T_or_u, du=None, p=None, dynamics_noise=True, measurement_noise=True, sample_initial=False, rng=None):
    """x, u, y = simulate(pf, T, du) / simulate(pf, u) — reference src/filtering.jl:457-477.  Host-side data
    generation (not part of the hot path); rng is a numpy Generator."""
    rng = np.random.default_rng(0) if rng is None else rng
    if np.isscalar(T_or_u):
        T = int(T_or_u)
        u = np.stack([du.rand(rng) for _ in range(T)]) if pf.nu else np.zeros((T, 0))
    else:
        u = np.asarray(T_or_u, dtype=np.float64).reshape(len(T_or_u), -1)
        T = u.shape[0]
    d0, df, dg = pf.initial_density, pf.dynamics_density, pf.measurement_density
    x = np.zeros((T, pf.nx))
    y = np.zeros((T, pf.ny))
    x[0] = d0.rand(rng) if sample_initial else d0.mean
    for t in range(T):
        ti = t * pf.Ts
        g = pf.measurement(x[t], u[t], p, ti)
        y[t] = g + (dg.rand(rng) if measurement_noise else 0.0)
        if t + 1 < T:
            if isinstance(pf.dynamics, QuadTankDynamics):
                fx = pf.dynamics(x[t], u[t], p, ti, pf.Ts)
            else:
                fx = pf.dynamics(x[t], u[t], p, ti)
            x[t + 1] = fx + (df.rand(rng) if dynamics_noise else 0.0)
    return x, u, y


def _sim_inputs(nu, T_or_u, M, du, u_per_trajectory, rng, lead=()):
    """the inputs of simulate_batch: (T, u) with u [T, nu], or lead + [M, T, nu] with u_per_trajectory"""
    if np.isscalar(T_or_u):
        T = int(T_or_u)
        if nu == 0:
            return T, np.zeros(lead + (M, T, 0) if u_per_trajectory else (T, 0))
        if du is None:
            raise ValueError("the model has inputs: pass du (their distribution) or the inputs themselves")
        rng = np.random.default_rng(0) if rng is None else rng
        if not u_per_trajectory:          # as simulate draws them
            return T, np.stack([du.rand(rng) for _ in range(T)])
        z = rng.standard_normal(lead + (M, T, nu))
        return T, du.mean + z @ np.linalg.cholesky(du.cov).T
    u = np.asarray(T_or_u, dtype=np.float64)
    if u_per_trajectory:
        if nu == 0:
            T = u.shape[len(lead) + 1]
            return T, np.zeros(lead + (M, T, 0))
        u = u.reshape(lead + (M, -1, nu))
        return u.shape[-2], u
    u = u.reshape(u.shape[0], -1)
    if u.shape[1] != nu:
        raise ValueError("u must be [T, %d]" % nu)
    return u.shape[0], u


def _sim_flags(dynamics_noise, measurement_noise, sample_initial):
    return ((_capi.SIM_DYNAMICS_NOISE if dynamics_noise else 0) | (_capi.SIM_MEASUREMENT_NOISE if measurement_noise else 0) |
            (_capi.SIM_SAMPLE_INITIAL if sample_initial else 0))


def simulate_batch(pf, T_or_u, M, du=None, *, seed=0, step0=0, dynamics_noise=True, measurement_noise=True, sample_initial=False, states=True,
                   u_per_trajectory=False, t_index0=0.0, rng=None):
    """x, u, y = simulate_batch(pf, T, M, du) / simulate_batch(pf, u, M): M trajectories of simulate(pf, T, du) (reference
    src/filtering.jl:457-477) at once, on the device (llpf_simulate), for every model the filter can run — device snippets without a
    host version, UserNoise / UserInitial included; not the Rao-Blackwellized filter.

    x [T, M, nx] (None with states=False), y [T, M, ny].  u: [T, nu] shared by all trajectories, drawn on the host from du as simulate
    draws them (rng: a numpy Generator, default seeded 0), or given; with u_per_trajectory [M, T, nu].  Step t runs at time
    (t_index0 + t) * Ts.  The noise comes from the engine's own generator under the key `seed` (derived as the filter derives its own):
    trajectory m is particle m of a filter with that seed that never resamples — its reset! draw for x_0 with sample_initial (else
    x_0 = mean(initial_density)), its predict! noise at Philox step step0 + t.  Measurement noise is drawn from the Gaussian
    measurement_density, also for a model with a likelihood of its own.  The filter itself is not changed."""
    T, u = _sim_inputs(pf.nu, T_or_u, int(M), du, u_per_trajectory, rng)
    x, y = pf._h.simulate(M, T, u, u_per_trajectory, t_index0, seed, step0, _sim_flags(dynamics_noise, measurement_noise, sample_initial),
                          states=states)
    return x, u, y


# ---------------------------------------------------------------------------------------------------
# banks of independent filters (parameter sweeps; reference test/runtests.jl:412-417)
# ---------------------------------------------------------------------------------------------------
class FilterBank:
    """n independent filters sharing N, model family and dimensions, batched into single launches.
    `filters_spec` is a list of (dynamics, measurement, df, dg, d0) tuples."""

    def __init__(self, N, filters_spec, *, resample_threshold=0.1, resampling_strategy=ResampleSystematic,
                 rng=None, Ts=1.0, device=0):
        models = [_build_model(dy, me, df, dg, d0, Ts) for (dy, me, df, dg, d0) in filters_spec]
        self.Ts = float(Ts)
        self.N = int(N)
        self.rng = 0 if rng is None else int(rng)
        cfg = S.make_config(models[0], N, S.PARTICLE_FILTER, resampling_strategy.code, resample_threshold, self.rng, device)
        self._h = _capi.BankHandle(cfg, models)
        self._models = models
        self.n_filters = len(models)

    def set_parameters(self, filters_spec):
        """new (dynamics, measurement, df, dg, d0) for every filter of the bank, nothing reallocated (llpf_bank_set_models)"""
        self.set_models([_build_model(dy, me, df, dg, d0, self.Ts) for (dy, me, df, dg, d0) in filters_spec])

    def set_models(self, models):
        """the same with llpf_model structs already built (metropolis_bank checks every candidate by building it, and hands that model on)"""
        models = list(models)
        self._h.set_models(models)
        self._models = models

    def loglik(self, u, y):
        """[loglik(pf_k, u, y) for k] — reference src/smoothing.jl:227-230 applied to every filter."""
        self._h.reset()
        return self._h.run(u, y, t_index0=1.0)["ll"]

    def forward(self, u, y, ll_steps=False):
        self._h.reset()
        return self._h.run(u, y, t_index0=0.0, ll_steps=ll_steps)

    def simulate(self, T_or_u, M, du=None, *, seed=0, step0=0, dynamics_noise=True, measurement_noise=True, sample_initial=False, states=True,
                 u_per_trajectory=False, t_index0=0.0, rng=None):
        """x, u, y = simulate_batch of every filter of the bank, filter k with its own parameters and the key seed + k (llpf_bank_simulate):
        x [F, T, M, nx] (None with states=False), y [F, T, M, ny]; u [T, nu] shared, or [F, M, T, nu] with u_per_trajectory."""
        T, u = _sim_inputs(self._h.nu, T_or_u, int(M), du, u_per_trajectory, rng, lead=(self.n_filters,) if u_per_trajectory else ())
        x, y = self._h.simulate(M, T, u, u_per_trajectory, t_index0, seed, step0, _sim_flags(dynamics_noise, measurement_noise, sample_initial),
                                states=states)
        return x, u, y
