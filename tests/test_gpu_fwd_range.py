"""The forward substitution of a reusing step through the kept slack and lambda_e panels in one launch (k_fwd_range, DESIGN.md
section 5).

Behind the x prefix a reusing step keeps the closed-form slack panels and the lambda_e groups.  PYIPM_FWD_RANGE=0 (read when the
handle is created) sends the right-hand side through them panel by panel -- k_fwd_diag, k_fwd_gemv, k_diag_apply each --, otherwise
one k_fwd_range launch and one k_diag_apply over their tiles do.  Both subtract the same products in the same order, so every
comparison is BIT FOR BIT: the direction as int64 patterns and every statistics field, over three steps of one handle (a recording
one, two reusing ones) with other s, lambda, mu and right-hand side each time.  reuse_info() says that steps 1 and 2 reused and
that the second snapshot exists where the case needs one; one child process reads PYIPM_GROUP_TRACE for where the launch ran.
The shape "resident" gives the one owner of a two-workgroup grid 18 chunks, two more than FWDP_RESIDENT = 16 slots.
All of it in the suite's NaN-filled workspace.  No test provokes a timeout: the error path is reviewed by reading."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = 3
# name: (n, me, mi), nb, group, second level?, the trace line in front of the launch's mark and the mark's group (None: no launch)
SHAPES = {
    "slack_and_two_groups": ((256, 256, 256), 128, 1, True, ("fwd prefix end", 2)),     # slack + two lambda_e groups in one range
    "group_straddles_n": ((384, 512, 384), 128, 2, True, ("diagonal blocks begin", 3)),  # a factored group in [gB, gS): lambda_e alone
    "group_straddles_e_i": ((256, 384, 256), 128, 2, True, ("fwd prefix end", 1)),       # panels 6, 7 are factored: per panel
    "odd_multiple_of_128": ((256, 256, 192), 128, 1, True, ("diagonal blocks begin", 4)),  # Npad = 896; panels straddle both borders
    "no_whole_group": ((256, 128, 256), 128, 2, False, None),
    "me0": ((256, 0, 256), 128, 1, False, None),
    "nb256": ((1024, 512, 512), 256, 2, True, ("fwd prefix end", 2)),                    # four-tile panels: the KC = 64 owner
    "resident": ((256, 256, 1024), 128, 1, True, ("fwd prefix end", 2)),                 # 18 owned chunks
}
FIRST, LAST = "slack_and_two_groups", "nb256"


def _qp(shape):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=11)


def _vec(qp, k, s_scale=1.0):
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(3000 + k)
    return dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
                ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=s_scale * qp["s"] * rng.uniform(0.5, 2.0, mi),
                lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.3 / (k + 1))


def _core(name, one_launch, opts=(), lam_e=True):
    from pyipm_amd.newton import NewtonCore
    shape, nb, group = SHAPES[name][:3]
    env = {"PYIPM_FWD_RANGE": "1" if one_launch else "0", "PYIPM_REUSE_LAM_E": "1" if lam_e else "0"}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                      # (read when the handle is created)
    try:
        core = NewtonCore(shape[0], shape[1], shape[2], device=0, nb=nb)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    core.set_option("expert", 1)
    core.set_option("group", group)
    for k, v in opts:                   # (before the first step: any set_option call drops a recorded prefix)
        core.set_option(k, v)
    return core


def _run(name, one_launch, opts=(), scales=(1.0, 1.0, 1.0), lam_e=True):
    """STEPS steps of one handle: [(dz bits, statistics)] and the snapshots' bytes; each step of the kind it is meant to be."""
    import torch
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    qp = _qp(SHAPES[name][0])
    core = _core(name, one_launch, opts, lam_e)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    out = []
    for k in range(STEPS):
        v = _vec(qp, k, scales[k])
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, 0)
        info = core.reuse_info()
        assert info["reused"] == k and info["last"] == ("recording" if k == 0 else "reusing"), (name, k, info)
        out.append((dz.clone().view(torch.int64), st))
    nbytes = core.reuse_info()["snapshot_bytes"]
    core.close()
    return out, nbytes


_REF = {}


def _ref(name, opts=(), scales=(1.0, 1.0, 1.0)):
    """The per-panel forward substitution (PYIPM_FWD_RANGE=0) under the same options: computed once per key, never changed."""
    import torch
    key = (name, opts, scales)
    if key not in _REF:
        _REF[key] = _run(name, False, opts, scales)
        dzs = [d.view(torch.float64) for d, _ in _REF[key][0]]
        for k in range(STEPS - 1):      # a stale value cannot hide: every entry of step k + 1 is another number
            assert bool((dzs[k + 1] != dzs[k]).all()), (name, k)
        assert all(bool(d.isfinite().all()) for d in dzs)
    return _REF[key]


def _same(got, ref, what):
    import torch
    for k in range(STEPS):              # steps 1 and 2 are the reusing ones
        assert torch.equal(got[0][k][0], ref[0][k][0]), (what, k)
        assert got[0][k][1] == ref[0][k][1], (what, k, got[0][k][1], ref[0][k][1])
    assert got[1] == ref[1], (what, "snapshot bytes", got[1], ref[1])


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "resident"])
def test_same_bits_as_the_per_panel_forward(name):
    got = _run(name, True)
    _same(got, _ref(name), name)
    first_level = _run(name, True, lam_e=False)[1]              # the x prefix alone: one snapshot
    assert (got[1] > first_level) == SHAPES[name][3], (name, got[1], first_level)


@pytest.mark.parametrize("blocks", [2, 3, 5])
@pytest.mark.parametrize("name", [FIRST, LAST])
def test_small_grids(name, blocks):
    """2 workgroups: one owner takes every chunk; 3 and 5: the smallest strided ownerships."""
    opts = (("sweep_max_blocks", blocks),)
    _same(_run(name, True, opts), _ref(name, opts), (name, blocks))


def test_more_chunks_than_resident_slots():
    """One owner, 18 owned chunks (two lambda_e chunks, sixteen lambda_i chunks): the last two make the round trip on every visit."""
    opts = (("sweep_max_blocks", 2),)
    _same(_run("resident", True, opts), _ref("resident", opts), "resident")


@pytest.mark.parametrize("name", [FIRST, LAST])
def test_without_the_one_launch_sweeps_it_falls_back(name):
    opts = (("sweep_persist", 0),)
    _same(_run(name, True, opts), _ref(name, opts), (name, "sweep_persist=0"))


def test_another_sigma_between_the_reusing_steps():
    scales = (1.0, 1.0, 1.0e3)
    _same(_run(FIRST, True, scales=scales), _ref(FIRST, scales=scales), "sigma")


def test_the_group_trace_says_where_the_launch_ran():
    """The mark "fwd kept range end" of a reusing step: behind the prefix launch where the slack panels are part of the range, behind
    "diagonal blocks begin" where the range is the lambda_e groups alone, absent where nothing is kept behind the prefix, in a
    recording step and under PYIPM_FWD_RANGE=0."""
    code = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_fwd_range as t
for name in t.SHAPES:
    for one in (True, False):
        qp = t._qp(t.SHAPES[name][0])
        core = t._core(name, one)
        core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
        for k in range(2):
            sys.stderr.write("[case] %%s %%d %%d\n" %% (name, int(one), k)); sys.stderr.flush()
            v = t._vec(qp, k)
            core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
            core.step(0.0, 0.0, 0)
        core.close()
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, PYIPM_GROUP_TRACE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    case, lines = None, {}
    for line in out.stderr.splitlines():
        if line.startswith("[case] "):
            case = tuple(line.split()[1:])
            lines[case] = []
        elif case is not None and " us  " in line:
            lines[case].append(line.split(" us  ", 1)[1])
    for name, spec in SHAPES.items():
        where = spec[4]
        for one in ("1", "0"):
            for k in ("0", "1"):
                marks = lines[(name, one, k)]
                at = [i for i, m in enumerate(marks) if m.startswith("fwd kept range end")]
                if where is None or one == "0" or k == "0":
                    assert at == [], (name, one, k, marks)
                    continue
                assert len(at) == 1, (name, marks)
                assert marks[at[0]] == "fwd kept range end g%d" % where[1], (name, marks[at[0]])
                assert marks[at[0] - 1].startswith(where[0]), (name, marks[at[0] - 1])
