"""A reusing step keeps the factor of the groups wholly inside the lambda_e columns too (the second level).

Every step is compared BIT FOR BIT -- direction and every field of the statistics -- with one step of a fresh handle without any
reuse (PYIPM_REUSE_X=0) and with the same step of a handle that keeps the x prefix alone (PYIPM_REUSE_LAM_E=0).  Which level ran
is told from the bytes of the snapshots (pyipm_newton_reuse_info: the second level holds a second one) and, in one child process,
from the line PYIPM_GROUP_TRACE prints.  nb = 128, NaN-filled workspaces, other vectors before every step."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, me, mi), group, the kept lambda_e groups [gS, gE) or None where the second level does not apply
SHAPES = {
    "one_panel_groups": ((256, 256, 256), 1, (3, 5)),      # x | x | slack | e | e | i | i
    "groups_of_two": ((384, 512, 384), 2, (3, 5)),         # a group straddles column n; two lambda_e groups, two lambda_i groups
    "border_inside_a_group": ((256, 384, 256), 2, (2, 3)), # panels 6, 7 straddle lambda_e | lambda_i: factored, not kept
    "no_whole_group": ((256, 128, 256), 2, None),          # me = 128 with groups of two
    "me0": ((256, 0, 256), 1, None),
    "odd_multiple_of_128": ((256, 256, 192), 1, (4, 5)),   # Npad = 896; a panel straddles slack | lambda_e, one lambda_e | lambda_i
}
A = SHAPES["one_panel_groups"]


def _qp(shape, seed=3):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=seed)


def _vec(qp, k, s_scale=1.0):
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(2000 + k)
    return dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
                ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=s_scale * qp["s"] * rng.uniform(0.5, 2.0, mi),
                lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.2 / (k + 1))


def _core(shape, group, reuse_x=True, lam_e=True):
    from pyipm_amd.newton import NewtonCore
    env = {"PYIPM_REUSE_X": "1" if reuse_x else "0", "PYIPM_REUSE_LAM_E": "1" if lam_e else "0"}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                      # (read when the handle is created)
    try:
        core = NewtonCore(shape[0], shape[1], shape[2], device=0, nb=128)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    core.set_option("expert", 1)
    core.set_option("group", group)
    return core


def _stage(core, blocks):
    core.stage_blocks(blocks["d2L"], blocks["Je"], blocks["Ji"])


def _step(core, v, delta=0.0, delta_c=0.0, refine=0):
    core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
    return core.step(delta, delta_c, refine)


_REF = {}


def _fresh(shape, group, blocks, v, key, delta=0.0, delta_c=0.0, refine=0):
    """One step of a fresh handle that reuses nothing.  Computed once per key."""
    if key not in _REF:
        core = _core(shape, group, reuse_x=False)
        _stage(core, blocks)
        dz, st = _step(core, v, delta, delta_c, refine)
        assert core.reuse_info()["snapshot_bytes"] == 0
        _REF[key] = (dz.clone(), st)
        core.close()
    return _REF[key]


def _same(got, ref, what):
    import torch
    assert torch.equal(got[0].view(torch.int64), ref[0].view(torch.int64)), what
    assert got[1] == ref[1], (what, got[1], ref[1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_four_steps_equal_fresh_handles_and_the_first_level(name):
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    shape, group, kept = SHAPES[name]
    qp = _qp(shape, seed=5)
    core, first = _core(shape, group), _core(shape, group, lam_e=False)
    _stage(core, qp); _stage(first, qp)
    for k in range(4):
        v = _vec(qp, k)
        got, got1 = _step(core, v), _step(first, v)
        assert core.reuse_info()["reused"] == k == first.reuse_info()["reused"], (name, k, core.reuse_info())
        assert np.isfinite(got[0].cpu().numpy()).all()
        _same(got, _fresh(shape, group, qp, v, (name, k)), (name, k, "fresh"))
        _same(got, got1, (name, k, "first level"))
    extra = core.reuse_info()["snapshot_bytes"] - first.reuse_info()["snapshot_bytes"]
    if kept is None:
        assert extra == 0, (name, extra)
    else:
        assert extra > 0, name
    core.close(); first.close()


def test_the_group_trace_says_what_was_kept():
    """The trace line of a reusing step: how many groups it kept, and which.  The group that straddles the lambda_e | lambda_i border
    is factored; shapes without a whole group inside lambda_e keep the x prefix alone."""
    code = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_reuse_lam_e as t
for name, (shape, group, kept) in t.SHAPES.items():
    qp = t._qp(shape, seed=5)
    core = t._core(shape, group)
    t._stage(core, qp)
    for k in range(2):
        sys.stderr.write("[case] %%s step %%d\n" %% (name, k)); sys.stderr.flush()
        t._step(core, t._vec(qp, k))
    core.close()
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, PYIPM_GROUP_TRACE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    case, seen = None, {}
    for line in out.stderr.splitlines():
        if line.startswith("[case] "):
            case = tuple(line.split()[1::2])
        elif "] keeps " in line or "] records " in line:
            seen[case] = line
    for name, (shape, group, kept) in SHAPES.items():
        rec, reu = seen[(name, "0")], seen[(name, "1")]
        assert "records" in rec and "keeps" in reu, (name, rec, reu)
        want = "lambda_e [%d, %d)" % (kept if kept else (0, 0))
        assert rec.endswith(want) and reu.endswith(want), (name, rec, reu, want)
        gb = int(reu.split("x prefix [0, ")[1].split(")")[0])
        assert int(reu.split("keeps ")[1].split()[0]) == gb + (kept[1] - kept[0] if kept else 0), (name, reu)


def test_another_sigma_between_two_reusing_steps():
    """s scaled by 1e3 between two reusing steps: the diagonal of the lambda_i block changes by orders of magnitude, and the kept
    groups' products are rounded along another running value -- a saved diagonal would show here."""
    shape, group, _ = A
    qp = _qp(shape)
    core = _core(shape, group)
    _stage(core, qp)
    for k, scale in ((0, 1.0), (1, 1.0), (2, 1.0e3), (3, 1.0)):
        v = _vec(qp, k, scale)
        got = _step(core, v)
        assert core.reuse_info()["reused"] == k
        _same(got, _fresh(shape, group, qp, v, ("sigma", k)), ("sigma", k))
    core.close()


def test_what_drops_the_prefix_drops_the_kept_groups():
    shape, group, _ = A
    qp, qp2 = _qp(shape), _qp(shape, seed=8)
    core = _core(shape, group)
    _stage(core, qp)
    _step(core, _vec(qp, 0)); _step(core, _vec(qp, 1))
    assert core.reuse_info()["reused"] == 1
    got = _step(core, _vec(qp, 2), 0.0, 1e-6)                    # another delta_c: in full
    assert core.reuse_info()["last"] == "full"
    _same(got, _fresh(shape, group, qp, _vec(qp, 2), "delta_c", 0.0, 1e-6), "delta_c")
    _step(core, _vec(qp, 3)); _step(core, _vec(qp, 4))          # (full: other shifts than the step before; then recording)
    got = _step(core, _vec(qp, 5))
    assert core.reuse_info()["last"] == "reusing"
    _same(got, _fresh(shape, group, qp, _vec(qp, 5), "again"), "again")
    core.set_option("pivtol_rel", 1e-14)
    got = _step(core, _vec(qp, 6))
    assert core.reuse_info()["last"] == "recording"
    _same(got, _fresh(shape, group, qp, _vec(qp, 6), "set_option"), "set_option")
    _step(core, _vec(qp, 7))
    assert core.reuse_info()["last"] == "reusing"
    _stage(core, qp2)
    got = _step(core, _vec(qp2, 8))
    assert core.reuse_info()["last"] == "recording"
    _same(got, _fresh(shape, group, qp2, _vec(qp2, 8), "stage_blocks"), "stage_blocks")
    _step(core, _vec(qp2, 9))
    assert core.reuse_info()["last"] == "reusing"
    core.kkt_storage()                                           # (the pointer is out: every later step runs in full)
    got = _step(core, _vec(qp2, 10))
    assert core.reuse_info()["last"] == "full"
    _same(got, _fresh(shape, group, qp2, _vec(qp2, 10), "kkt_storage"), "kkt_storage")
    core.close()


def test_separate_phases():
    import torch
    shape, group, _ = A
    qp = _qp(shape)
    ref, core = _core(shape, group, reuse_x=False), _core(shape, group)
    _stage(ref, qp); _stage(core, qp)

    def phases(c, v):
        c.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        c.residual(); c.assemble(0.0, 0.0)
        st = c.factor()
        return c.solve(flip=True), st

    for k, kind in ((0, "recording"), (1, "reusing"), (2, "reusing")):
        dz_ref, st_ref = phases(ref, _vec(qp, k))
        dz, st = phases(core, _vec(qp, k))
        assert core.reuse_info()["last"] == kind
        assert st == st_ref and torch.equal(dz.view(torch.int64), dz_ref.view(torch.int64)), k
    v = _vec(qp, 3)                                              # the matrix between the phases is whole, lambda_e columns included
    for c in (ref, core):
        c.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        c.residual(); c.assemble(0.0, 0.0)
    assert torch.equal(core.kkt_storage().view(torch.int64), ref.kkt_storage().view(torch.int64))
    assert core.factor() == ref.factor()
    assert torch.equal(core.solve().view(torch.int64), ref.solve().view(torch.int64))
    ref.close(); core.close()


@pytest.mark.parametrize("refine", [2, -1])
def test_refinement_on_a_step_that_keeps_them(refine):
    shape, group, _ = A
    qp = _qp(shape)
    core = _core(shape, group)
    _stage(core, qp)
    _step(core, _vec(qp, 0))
    got = _step(core, _vec(qp, 1), refine=refine)
    assert core.reuse_info()["last"] == "reusing"
    _same(got, _fresh(shape, group, qp, _vec(qp, 1), ("refine", refine), refine=refine), refine)
    core.close()


def test_pivot_state_of_the_kept_groups():
    """An LP with equalities (d2L = 0: every x pivot is static, the multiplier blocks are built on the perturbed pivots) through
    three reusing steps that keep a lambda_e group -- its tile inverses, saved tiles and flags are those of the recording step.
    tests/golden/pivot_lp_eq.npz itself cannot get there: its lambda_e columns [416, 464) hold no whole panel at any panel width.
    pivot_lp_eq_wide.npz is the same recipe (oracle/make_golden.py: pivot_step, seed 26) at n, me, mi = 256, 128, 256, where
    panel 4 is lambda_e.  Against the oracle's direction with the bound and the inertia tests/test_gpu_pivoting.py holds
    pivot_lp_eq to, and against fresh handles bit for bit."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "pivot_lp_eq_wide.npz"))
    n, me, mi = int(d["nvar"]), int(d["neq"]), int(d["nineq"])
    assert (n, me, mi) == (256, 128, 256) and float(d["delta_out"]) == 0.0
    x, Q, Am, G = d["x"], d["Q"], d["A"], d["G"]
    blocks = dict(d2L=Q, Je=np.ascontiguousarray(Am.T), Ji=np.ascontiguousarray(G.T))
    v = dict(df=Q @ x + d["c"], ce=Am @ x - d["b"], ci=G @ x - d["h"], s=d["s"], lda=d["lda"], mu=float(d["mu"]))
    shape = (n, me, mi)
    core, first = _core(shape, 1), _core(shape, 1, lam_e=False)
    _stage(core, blocks); _stage(first, blocks)
    for k in range(4):
        dz, st = _step(core, v, refine=-1)
        _step(first, v, refine=-1)
        assert core.reuse_info()["reused"] == k
        _same((dz, st), _fresh(shape, 1, blocks, v, "lp_eq_wide", refine=-1), k)
        err = float(np.linalg.norm(dz.cpu().numpy() - d["dz"]) / np.linalg.norm(d["dz"]))
        print("pivot_lp_eq_wide step %d: rel. error against the oracle %.3e, statistics %s" % (k, err, st))
        assert err <= 1e-10, (k, err)
        assert st["n_neg"] == me + mi == int(d["neg"]) and st["n_zero"] == n and st["nonfinite"] == 0
    # the second level ran: a second snapshot of the size the kept group [cS, cE) = [512, 640) of Npad = 896 asks for
    rows = 896 - 640
    assert core.reuse_info()["snapshot_bytes"] - first.reuse_info()["snapshot_bytes"] == 8 * (32 + rows * 128 + rows * rows)
    core.close(); first.close()
