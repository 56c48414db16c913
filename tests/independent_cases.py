"""The cases of the independent numpy restatement (oracle/independent.py): the same systems expressed twice — as the numpy
objects that restatement takes and as the llpf_model the engine / the C oracle take — plus the Philox draws both are fed."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import independent as ind          # oracle/independent.py
import models as M
import rbfull_models as RM
from llpf_amd import _structs as S

STREAM_INIT, STREAM_DYNAMICS, STREAM_USER, STREAM_USER_INIT = 0, 1, 7, 8
SEED = 7


def _gauss(g):
    return ind.Gaussian(S.gaussian_mean(g), S.gaussian_cov_matrix(g))


def _mat(arr, r, c):
    return np.array(arr[:r * c], dtype=np.float64).reshape(r, c)


def _lg_objects(m):
    return ind.LinearModel(_mat(m.A, m.nx, m.nx), _mat(m.B, m.nx, m.nu) if m.nu else None, _mat(m.C, m.ny, m.nx))


def _qt_object(m):
    q = list(m.qt)
    return ind.QuadTank(k1=q[0], k2=q[1], g=q[2], A=tuple(q[3:7]), a=tuple(q[7:11]), gamma=tuple(q[11:13]), tswitch=q[13],
                        a1factor=q[14], eps=q[15], Ts=m.Ts, supersample=m.supersample)


def _lg_data(lg, T=60):
    """U, Y and Y with a missing measurement"""
    _, U, Yfull = M.simulate_lg(lg, T, seed=3)
    Y = Yfull.copy()
    Y[17] = np.nan
    return U, Yfull, Y


def _lg_filter(lg, N, thr, strat):
    return ind.ParticleFilter(N, _lg_objects(lg), _gauss(lg.dynamics_density), _gauss(lg.measurement_density), _gauss(lg.initial_density),
                              thr, strat == S.RESAMPLE_STRATIFIED, lg.Ts, residual=strat == S.RESAMPLE_RESIDUAL)


STRATEGIES = {"systematic": S.RESAMPLE_SYSTEMATIC, "stratified": S.RESAMPLE_STRATIFIED, "residual": S.RESAMPLE_RESIDUAL}
MODES = {"forward": 0, "loglik": 1}


def aux_cases():
    """The AuxiliaryParticleFilter cases (frozen as the others): name -> the dict of cases() with `aux` = the loop (0 forward_trajectory,
    1 loglik) and `wrap` (the plain filter -> the auxiliary one; the tests wrap it in misread variants).  Every case has a missing
    look-ahead measurement and an outlier that sends the engine's normalisations to their exact-maximum form."""
    out = {}
    lg = M.lg_test_model()
    U, _, Y = _lg_data(lg)                              # Y[17] is missing: the look-ahead of step 16
    Y = Y.copy()
    Y[31] += 11.0
    qt = M.quadtank_model()
    Uq, Yq = M.quadtank_data(40, seed=2)
    Yq = Yq.copy()
    Yq[9] = np.nan
    Yq[22] += 11.0
    for mname, mode in MODES.items():
        for sname, strat in STRATEGIES.items():
            out["aux_lg_%s_%s" % (sname, mname)] = dict(
                model=lg, kind=S.PARTICLE_FILTER, N=400, T=60, thr=0.1, strategy=strat, t0=0.0, U=U, Y=Y, aux=mode,
                make=lambda strat=strat: _lg_filter(lg, 400, 0.1, strat), wrap=ind.AuxiliaryParticleFilter)
        # over an AdvancedParticleFilter, from t = 485: the run crosses the quadruple tank's switch time (500)
        out["aux_quadtank_%s" % mname] = dict(
            model=qt, kind=S.ADVANCED_PARTICLE_FILTER, N=300, T=40, thr=0.5, strategy=S.RESAMPLE_SYSTEMATIC, t0=485.0, U=Uq, Y=Yq, aux=mode,
            make=lambda: ind.ParticleFilter(300, _qt_object(qt), _gauss(qt.dynamics_density), _gauss(qt.measurement_density),
                                            _gauss(qt.initial_density), 0.5, False, qt.Ts),
            wrap=lambda pf: ind.AuxiliaryParticleFilter(pf, advanced=True), advanced=True)
    return out


SIZES = (1, 2, 63, 64, 65, 1024, 1025, 2049)          # a tile of the kernels is 1024 particles: 1025 and 2049 leave one particle in the last
SIZE_STEPS = 6


def size_case(N, strategy, aux):
    """a short run at N particles, computed live: the residual filter at threshold 1.0 (aux None), or the auxiliary filter in loop `aux`"""
    lg = M.lg_test_model()
    _, U, Y = M.simulate_lg(lg, SIZE_STEPS + 1, seed=3)
    T = SIZE_STEPS if aux != 0 else SIZE_STEPS + 1      # forward_trajectory predicts T - 1 times
    case = dict(model=lg, kind=S.PARTICLE_FILTER, N=N, T=T, thr=1.0, strategy=strategy, t0=0.0, U=U[:T], Y=Y[:T],
                make=lambda: _lg_filter(lg, N, 1.0, strategy))
    if aux is not None:
        case.update(aux=aux, wrap=ind.AuxiliaryParticleFilter)
    return case


STANDALONE = ((10, 10), (9, 9), (1025, 1025), (4097, 300), (300, 4097))


def standalone_residual(n, m):
    """weights, uniforms and previous ancestors of one stand-alone residual resampling of n particles into m outputs"""
    rng = np.random.default_rng(n + m)
    we = rng.exponential(size=n) ** 3
    we /= we.sum()
    return we, rng.uniform(size=m), np.full(m, 5, dtype=np.int64)


def cases():
    """name -> dict(model (llpf_model), kind, N, T, thr, strategy, t0, U, Y, make (-> independent filter))"""
    out = {}
    lg = M.lg_test_model()
    U, Yfull, Y = _lg_data(lg)
    # residual resampling at threshold 1.0 without the missing row: there the weights are uniform, every nw_i is 1 +- 1 ulp and floor()
    # is decided by rounding alone (tests/test_gpu_residual.py keeps the exact test of that corner)
    for name, thr, strat, Yc in (("pf_lg_systematic", 0.5, S.RESAMPLE_SYSTEMATIC, Y), ("pf_lg_stratified", 1.0, S.RESAMPLE_STRATIFIED, Y),
                                 ("pf_lg_residual", 0.5, S.RESAMPLE_RESIDUAL, Y), ("pf_lg_residual_thr1", 1.0, S.RESAMPLE_RESIDUAL, Yfull)):
        out[name] = dict(model=lg, kind=S.PARTICLE_FILTER, N=400, T=60, thr=thr, strategy=strat, t0=0.0, U=U, Y=Yc,
                         make=lambda thr=thr, strat=strat: _lg_filter(lg, 400, thr, strat))
    # measurement likelihoods of the user's own (run-time compiled on the engine side, tests/user_models.py): Laplace and Student-t
    # noise on the same linear system; `user` = (oracle kind, oracle parameters, device snippet, qt parameter block of the snippet)
    import user_models as UM
    st = ind.StudentT(4.0, 0.7)
    for name, dens, user in (("pf_lg_laplace", ind.Laplace(0.8), (1, [0.8], UM.LAPLACE_SRC, [0.8])),
                             ("pf_lg_student_t", st, (2, [4.0, 0.7, st.c1], UM.STUDENT_T_SRC, [4.0, 0.7, st.c1]))):
        out[name] = dict(model=lg, kind=S.ADVANCED_PARTICLE_FILTER, N=400, T=60, thr=0.5, strategy=S.RESAMPLE_SYSTEMATIC, t0=0.0, U=U, Y=Y, user=user,
                         make=lambda dens=dens: ind.ParticleFilter(400, _lg_objects(lg), _gauss(lg.dynamics_density), dens, _gauss(lg.initial_density), 0.5, False, lg.Ts))
    # process noise / initial density of the model's own (UserModel::noise / ::initial): `noise` = (oracle kind, oracle parameters),
    # `initial` likewise, `user` = (-, -, device snippet, qt parameter block)
    box = ([-1.0, 0.5], [3.0, 2.5])
    for name, dfo, d0o, extra in (
            ("pf_lg_mult_noise_box", ind.MultiplicativeGaussianNoise(0.1, 0.25), ind.UniformBox(*box),
             dict(noise=(1, [0.1, 0.25]), initial=(1, box[0] + box[1]), user=(0, [], UM.MULT_NOISE_BOX_SRC, [0.1, 0.25] + box[0] + box[1]))),
            ("pf_lg_laplace_noise", ind.LaplaceNoise(0.2), _gauss(lg.initial_density),
             dict(noise=(2, [0.2]), user=(0, [], UM.LAPLACE_NOISE_SRC, [0.2])))):
        out[name] = dict(model=lg, kind=S.ADVANCED_PARTICLE_FILTER, N=400, T=60, thr=0.5, strategy=S.RESAMPLE_SYSTEMATIC, t0=0.0, U=U, Y=Y,
                         make=lambda dfo=dfo, d0o=d0o: ind.ParticleFilter(400, _lg_objects(lg), dfo, _gauss(lg.measurement_density), d0o, 0.5, False, lg.Ts), **extra)
    qt = M.quadtank_model()
    Uq, Yq = M.quadtank_data(40, seed=2)
    out["pf_quadtank"] = dict(model=qt, kind=S.ADVANCED_PARTICLE_FILTER, N=300, T=40, thr=0.5, strategy=S.RESAMPLE_SYSTEMATIC, t0=485.0, U=Uq, Y=Yq,
                              make=lambda: ind.ParticleFilter(300, _qt_object(qt), _gauss(qt.dynamics_density), _gauss(qt.measurement_density),
                                                              _gauss(qt.initial_density), 0.5, False, qt.Ts))
    for shape in ((1, 2, 1), (2, 2, 2), (4, 8, 2), "quadtank"):
        if shape == "quadtank":
            m = RM.quadtank_case()
            name = "rb_quadtank_4_8_2"
        else:
            m, _ = RM.linear_case(*shape, seed=1, state_dependent=True)
            name = "rb_linear_%d_%d_%d" % shape
        Ur, Yr = RM.simulate_io(m, 20, seed=4)
        nn, nl, ny, nu = m.nx, m.rb.nxl, m.ny, m.nu

        def make(m=m, nn=nn, nl=nl, ny=ny, nu=nu):
            An = np.array([list(m.rb.An[k][:nn * nl]) for k in range(nn + 1)]).reshape(nn + 1, nn, nl)
            fn = _qt_object(m) if m.rb.fn_kind == 1 else ind.LinearModel(_mat(m.A, nn, nn), _mat(m.B, nn, nu) if nu else None, _mat(m.C, ny, nn))
            return ind.RBPF(200, fn, An, _mat(m.rb.Al, nl, nl), _mat(m.rb.Bl, nl, nu) if nu else None, _mat(m.rb.Cl, ny, nl),
                            _gauss(m.dynamics_density), S.gaussian_cov_matrix(m.linear_noise), _gauss(m.measurement_density),
                            _gauss(m.initial_density), _gauss(m.linear_initial), 0.5, False, m.Ts)
        out[name] = dict(model=m, kind=S.PARTICLE_FILTER, N=200, T=20, thr=0.5, strategy=S.RESAMPLE_SYSTEMATIC, t0=0.0, U=Ur, Y=Yr, make=make, rb=True)
    return out


def draws(ob, case):
    """the Philox draws a fresh handle consumes: reset! number 1 (the constructor took number 0), predict! numbers 0, 1, ..."""
    nd = case["model"].nx

    def normals(step, n, k):
        return ob.normals(SEED, step, STREAM_DYNAMICS, nd, n)[:, :k]

    def uniforms(step, n):
        return ob.resample_uniforms(case["strategy"], n, SEED, step)

    return ob.normals(SEED, 1, STREAM_INIT, nd, case["N"]), normals, uniforms


def _residual_calls(pf):
    """the margins of every residual resampling of a run next to their slacks, [calls, 4]: int_margin, slack_int, edge_margin, slack_edge"""
    return np.array([[c["int_margin"], c["slack_int"], c["edge_margin"], c["slack_edge"]] for c in pf.calls]).reshape(-1, 4)


def run_independent(ob, case, wrap=None):
    """wrap: used in place of the case's own for an auxiliary case (a misread variant of the restatement)"""
    f = case["make"]()
    xi0, normals, uniforms = draws(ob, case)
    nd = case["model"].nx
    if case.get("aux") is not None:
        a = (wrap or case["wrap"])(f)
        a.reset(xi0)
        ll_steps, nres = a.run(case["U"], case["Y"], case["aux"], normals, uniforms, t_index0=case["t0"])
        return dict(ll_steps=ll_steps, resamples=np.int64(nres), anc_final=np.asarray(f.j, dtype=np.int64), x_final=f.x, w_final=f.w,
                    residual_calls=_residual_calls(f))
    if case["strategy"] == S.RESAMPLE_RESIDUAL:
        f.reset(xi0)
        ll_steps, nres = f.run(case["U"], case["Y"], case["t0"], normals, uniforms)
        return dict(ll_steps=ll_steps, resamples=np.int64(nres), anc_final=np.asarray(f.j, dtype=np.int64), x_final=f.x, w_final=f.w,
                    residual_calls=_residual_calls(f))
    if case.get("initial"):
        f.reset(xi0, ob.uniforms_nd(SEED, 1, STREAM_USER_INIT, nd, case["N"]))
    else:
        f.reset(xi0)
    if case.get("noise"):
        ll_steps, nres = f.run(case["U"], case["Y"], case["t0"], normals, uniforms,
                               user_uniforms=lambda step, n, k: ob.uniforms_nd(SEED, step, STREAM_USER, nd, n)[:, :k])
    else:
        ll_steps, nres = f.run(case["U"], case["Y"], case["t0"], normals, uniforms)
    res = dict(ll_steps=ll_steps, resamples=np.int64(nres), anc_final=np.asarray(f.j, dtype=np.int64))
    if case.get("rb"):
        res.update(x_final=np.hstack([f.xn, f.xl]), R_final=f.R)
    else:
        res.update(x_final=f.x)
    return res


def run_handle(h, case):
    """(the per-step log-likelihoods, the number of predict! calls that resampled) of a case on the C oracle or the engine (one set of
    verbs), after reset.  The run loops of the auxiliary filter count time from 0; a case that starts elsewhere is driven step by step, as
    AuxiliaryParticleFilter.run is, and its resamplings are counted step by step too (the engine's counter is that of its last run)."""
    U, Y, T, Ts = case["U"], case["Y"], case["T"], case["model"].Ts
    if case.get("aux") is None:
        return h.run(U, Y, case["t0"], ll_steps=True)["ll_steps"], h.resample_count()
    if case["t0"] == 0.0:
        return h.run_aux(U, Y, case["aux"], ll_steps=True)["ll_steps"], h.resample_count()
    ll = np.zeros(T)
    nres = 0
    for k in range(T):
        t = (case["t0"] + k) * Ts
        if case["aux"] == 1 and k == T - 1:
            ll[k] = h.update(U[k], Y[k], t)
        else:
            ll[k] = h.aux_correct()
            if k == T - 1:
                break
            h.aux_predict(U[k], None if np.any(np.isnan(Y[k + 1])) else Y[k + 1], t)
        nres += int(h.last_resampled())
    return ll, nres


def config_of(case):
    return S.make_config(case["model"], case["N"], case["kind"], case["strategy"], case["thr"], SEED, 0)


def oracle_of(ob, case, order):
    """the C oracle for a case (with the case's own measurement likelihood installed)"""
    o = ob.OracleFilter(config_of(case), order)
    if case.get("user") and case["user"][0]:
        o.set_user_loglik(case["user"][0], case["user"][1])
    if case.get("noise"):
        o.set_user_noise(*case["noise"])
    if case.get("initial"):
        o.set_user_initial(*case["initial"])
    return o


def engine_of(case):
    """the HIP engine for a case: cases with a measurement likelihood of their own run a model compiled from the case's device snippet"""
    from llpf_amd import _capi
    if not case.get("user"):
        return _capi.FilterHandle(config_of(case))
    kind, par, src, qt = case["user"]
    m = S.Model.from_buffer_copy(bytes(case["model"]))
    m.model_id = _capi.model_compile(src, m.nx, m.ny)
    for i, v in enumerate(qt):
        m.qt[i] = v
    return _capi.FilterHandle(S.make_config(m, case["N"], case["kind"], case["strategy"], case["thr"], SEED, 0))
