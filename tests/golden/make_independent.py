"""Freezes the outputs of the INDEPENDENT numpy restatement (oracle/independent.py — shares no code with the engine or with
oracle/llpf_oracle.c) on the cases of tests/independent_cases.py as tests/golden/indep_<case>.npz, and prints how far the C
oracle's two orders are from them.  These are NOT reference outputs (Julia cannot run in this image): they pin the C oracle and
the engine against a second restatement of the same reference lines, in particular the per-particle Riccati / Kalman recursion
of the Rao-Blackwellized filter (src/rbpf.jl:206-221, src/filtering.jl:100-128), which oracle and engine share as one header.
    python tests/golden/make_independent.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import independent_cases as IC
import oracle_binding as ob

only = sys.argv[1:]                 # case names; none: every case
for name, case in {**IC.cases(), **IC.aux_cases()}.items():
    if only and name not in only:
        continue
    r = IC.run_independent(ob, case)
    np.savez_compressed(os.path.join(HERE, "indep_%s.npz" % name), U=case["U"], Y=case["Y"], **r)
    line = "%-26s resamples %2d" % (name, int(r["resamples"]))
    for tag, order in (("reference order", ob.ORDER_REFERENCE), ("device order", ob.ORDER_DEVICE)):
        o = IC.oracle_of(ob, case, order)
        o.reset()
        ll, _ = IC.run_handle(o, case)
        line += " | %s: max|dll| %.1e max|dx| %.1e anc %s" % (tag, np.max(np.abs(ll - r["ll_steps"])),
                                                            np.max(np.abs(o.particles() - r["x_final"])), np.array_equal(o.ancestors(), r["anc_final"]))
        if case.get("rb"):
            line += " max|dR| %.1e" % np.max(np.abs(o.rb_linear_state()[1] - r["R_final"]))
        if "w_final" in r:
            line += " max|dw| %.1e" % np.max(np.abs(o.weights() - r["w_final"]))
    c = r.get("residual_calls")
    if c is not None and len(c):    # the two closest calls of the run's residual resamplings, each next to its slack
        ki, ke = int(np.argmin(c[:, 0])), int(np.argmin(c[:, 2]))
        with np.errstate(invalid="ignore"):
            ratio = min(np.nanmin(c[:, 0] / c[:, 1]), np.nanmin(c[:, 2] / c[:, 3]))
        line += " | residual: %d calls, integer margin %.1e (slack %.1e), edge margin %.1e (slack %.1e), margin / slack >= %.1e" % (
            len(c), c[ki, 0], c[ki, 1], c[ke, 2], c[ke, 3], ratio)
    print(line)
