"""Forward-mode differentiation of a traced callable's expression DAG (tracing.jacobian, emit_user_model(..., jacobians=True)): the
derivative rules of every node kind against central differences, the pruning of structural zeros, the value part of `dynamics_jac` as
the very statements of `dynamics`, and what hiprtc and llpf_model_traits make of the emitted members (LLPF_JIT_COMPILE_ONLY: nothing
runs, no GPU needed)."""
import re

import numpy as np

from llpf_amd import _capi, _structs as S, tracing as tr
import ekf_common as ec

Q = dict(S.QUADTANK_DEFAULTS)
# the bar of a central difference with h = 1e-6 on entries of order 1: its roundoff is ~ eps |f| / h ~ 1e-9 and its truncation h^2 f''' / 6
# smaller still, while a wrong rule is wrong by the entry's own size
FD_BAR = 1e-7


def every_kind(x, u, p, t):
    """every node kind of the tracer: add sub mul div neg abs sqrt exp log log1p sel, integer powers, maximum / minimum, u and t"""
    a = tr.sqrt(x[0] * x[0] + 2.0) - tr.exp(-0.5 * x[1]) * u[0]
    b = tr.ifelse(x[0] > 0.5, x[0] ** 3 * 0.1, tr.log(x[1] * x[1] + 3.0)) / (1.0 + abs(x[1]))
    c = tr.log1p(x[2] * x[2]) + tr.maximum(x[0], x[2]) - tr.minimum(x[1], 0.3) + t * 0.01
    d = (-x[2]) ** 4 * 0.01 + abs(x[0] - x[1]) / (2.0 + x[2] ** 2)
    return [a, b + d, c]


def _generic_points(n, seed):
    """points of [-2, 2]^3 at least 0.05 away from every kink of every_kind: x0 = 0.5, x1 = 0, x0 = x2, x1 = 0.3, x0 = x1"""
    rng = np.random.default_rng(seed)
    pts, branches = [], set()
    while len(pts) < n:
        x = rng.uniform(-2.0, 2.0, 3)
        if min(abs(x[0] - 0.5), abs(x[1]), abs(x[0] - x[2]), abs(x[1] - 0.3), abs(x[0] - x[1])) < 0.05:
            continue
        pts.append(x)
        branches.add((x[0] > 0.5, x[1] < 0, x[0] > x[2], x[1] < 0.3, x[0] < x[1]))
    assert len(branches) >= 12, "both branches of every sel and both signs of every abs are visited"
    return pts


def test_every_rule_against_central_differences():
    """1. evaluate() of the Jacobian nodes against central differences of evaluate() of the value nodes at 100 generic points"""
    g, outs = tr.trace(every_kind, 3, 1)
    kinds = {n[0] for n in g.nodes}
    assert {"add", "sub", "mul", "div", "neg", "abs", "sqrt", "exp", "log", "log1p", "sel"} <= kinds, kinds
    n_value = len(g.nodes)
    J = tr.jacobian(g, outs, 3)
    assert all(n[0] != "x" for n in g.nodes[n_value:]) and J[0][2] is None, "a is independent of x2: no node"
    worst = 0.0
    for x in _generic_points(100, 0):
        u, t = [0.7], 3.0
        got = np.array(tr.evaluate(g, J, x, u, t))
        want = ec.central_differences(lambda z: tr.evaluate(g, outs, z, u, t), list(x), 3)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.all(np.abs(got - want) <= FD_BAR), (x, got, want)
    print("every node kind: worst |autodiff - central difference| %.2e" % worst)
    # evaluate() runs only what the outputs depend on: the third output reads neither u nor y, so neither has to be given
    x = [0.3, -1.1, 0.9]
    assert tr.evaluate(g, [outs[2]], x, t=3.0) == tr.evaluate(g, [outs[2]], x, [0.7], 3.0)
    assert tr.evaluate(g, [J[2]], x, t=3.0) == tr.evaluate(g, [J[2]], x, [0.7], 3.0)


def _quadtank_points(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0.05, 6.0, 4), [0.5 * rng.random(), 0.5 * rng.random()], t) for t in (3.0, 499.5, 500.0, 777.0) for _ in range(n // 4)]


def test_the_traced_quadtank_and_its_structural_zeros():
    """2. the traced quad-tank (rk4 of the tank equations, two sub-steps) against central differences; 10 of the 16 entries are
    structurally zero, stored as the literal 0.0, and nothing in the text multiplies by a zero constant"""
    f = tr.rk4(ec.quadtank_rhs, 1.0, 2)
    g, outs = tr.trace(f, 4, 2, p=Q)
    J = tr.jacobian(g, outs, 4)
    assert [[e is not None for e in row] for row in J] == [[True, False, True, False], [False, True, False, True], [False, False, True, False],
                                                         [False, False, False, True]]
    worst = 0.0
    for x, u, t in _quadtank_points(100, 1):
        got = np.array(tr.evaluate(g, J, x, u, t))
        want = ec.central_differences(lambda z: tr.evaluate(g, outs, z, u, t), list(x), 4)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.all(np.abs(got - want) <= FD_BAR), (x, t, got, want)
    print("traced quad-tank: worst |autodiff - central difference| %.2e" % worst)
    src = tr.emit_user_model(4, 2, 2, f, ec.quadtank_levels, p=Q, jacobians=True)
    body = src[src.index("DEV void dynamics_jac"):src.index("DEV void measurement_jac")]
    assert len(re.findall(r"J\[\d+\] = 0\.0;", body)) == 10 and len(re.findall(r"J\[\d+\] = v\d+;", body)) == 6
    mbody = src[src.index("DEV void measurement_jac"):]
    assert len(re.findall(r"J\[\d+\] = 0\.0;", mbody)) == 6 and len(re.findall(r"J\[\d+\] = c\d+;", mbody)) == 2
    zero_consts = set(re.findall(r"const double (c\d+) = llpf_u2d\(0x[08]000000000000000ULL\)", src))
    for line in src.split("\n"):
        m = re.search(r"= \((\w+(?:\[\d\])?) \* (\w+(?:\[\d\])?)\);", line)
        if m:
            assert m.group(1) not in zero_consts and m.group(2) not in zero_consts, line


def _statements(src, member):
    body = src[src.index("DEV void " + member + "("):]
    return [line.strip() for line in body[body.index("{") + 1:body.index("\n    }")].strip().split("\n")]


def test_the_value_part_is_the_statement_list_of_the_value_member():
    """3. the derivative nodes are appended to the graph of the value: `dynamics_jac` begins with the statements of `dynamics` (same node
    ids, same text), then continues; likewise the measurement"""
    for fn, meas, nx, nu, ny, p in ((tr.rk4(ec.quadtank_rhs, 1.0, 2), ec.quadtank_levels, 4, 2, 2, Q),
                                    (every_kind, lambda x, u, p, t: [x[0] * x[2], tr.exp(x[1])], 3, 1, 2, None)):
        src = tr.emit_user_model(nx, nu, ny, fn, meas, p=p, jacobians=True)
        for member, out, val in (("dynamics", "out", "fx"), ("measurement", "out", "gx")):
            plain = _statements(src, member)
            jac = _statements(src, member + "_jac")
            n_val = len([s for s in plain if not s.strip().startswith(out + "[")])
            assert (n_val > 0 or member == "measurement") and jac[:n_val] == plain[:n_val], member
            assert [s.replace(out + "[", val + "[") for s in plain[n_val:]] == [s for s in jac if s.strip().startswith(val + "[")], member
        # the default emits the text it always did: the jacobians=True snippet is that text with the two members appended
        base = tr.emit_user_model(nx, nu, ny, fn, meas, p=p)
        assert "_jac" not in base and src.startswith(base[:base.rindex("};")])


# what the parent commit emits for this two-line model (kept literally: existing traced models keep their source and cache entries)
TWO_LINE_EXPECTED = """struct UserModel {
    static constexpr bool RB = false;
    double u_[1];
    double t_;
    DEV void prepare(const ModelD* m, const double* u, double t) {
        for (int j = 0; j < 0; ++j) u_[j] = (u != nullptr) ? u[j] : 0.0;
        t_ = t;
    }
    DEV void dynamics(const double* x, double* out) const {
        const double c2 = llpf_u2d(0x3feccccccccccccdULL) /* 0.9 */;
        const double v3 = (c2 * x[0]);
        out[0] = v3;
    }
    DEV void measurement(const double* x, double* out) const {
        const double v2 = (x[0] * x[0]);
        out[0] = v2;
    }
};
"""


def test_hiprtc_accepts_the_members_and_the_traits_report_them(monkeypatch):
    """4. compile only: the jacobians=True snippet has both new trait bits, the default snippet neither (and is the parent's text), a
    snippet with one member reports that one"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    f, g = (lambda x, u, p, t: [0.9 * x[0]]), (lambda x, u, p, t: [x[0] * x[0]])
    base = tr.emit_user_model(1, 0, 1, f, g)
    assert base == TWO_LINE_EXPECTED
    both = _capi.TRAIT_DYNAMICS_JAC | _capi.TRAIT_MEASUREMENT_JAC
    assert (_capi.TRAIT_DYNAMICS_JAC, _capi.TRAIT_MEASUREMENT_JAC) == (16, 32)
    assert _capi.model_traits(_capi.model_compile(base, 1, 1)) == 0
    assert _capi.model_traits(_capi.model_compile(tr.emit_user_model(1, 0, 1, f, g, jacobians=True), 1, 1)) == both
    qt = tr.emit_user_model(4, 2, 2, tr.rk4(ec.quadtank_rhs, 1.0, 2), ec.quadtank_levels, p=Q, jacobians=True)
    assert _capi.model_traits(_capi.model_compile(qt, 4, 2)) == both
    assert _capi.model_traits(_capi.model_compile(tr.emit_user_model(3, 1, 2, every_kind, None, jacobians=True), 3, 2)) == both
    assert _capi.model_traits(_capi.model_compile(ec.SQUARE_DYN_JAC_ONLY_SRC, 1, 1)) == _capi.TRAIT_DYNAMICS_JAC
    assert _capi.model_traits(_capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)) == both
    d = tr.traced_dynamics(f, 1, 0, measurement=g, ny=1, jacobians=True)
    assert "dynamics_jac" in d.src and "dynamics_jac" not in tr.traced_dynamics(f, 1, 0, measurement=g, ny=1).src
