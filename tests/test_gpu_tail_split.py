"""The tail split of a reusing step (StepPlan::tail_split).

Where one tile-chain group hands over to the next, the chain's launch takes the rows of the next diagonal block along, the head
runs as the diagonal block's share on the next chain's stream and the rest beside it, and all rows kernels leave the chain's
stream.  PYIPM_TAIL_SPLIT=0 (read when the handle is created) keeps the old order.  No product and no order of products per
entry changes, so every comparison is BIT FOR BIT against a handle created with PYIPM_TAIL_SPLIT=0: the direction as int64
patterns, every statistics field and, behind the last step, the lower triangle of the factor storage.  Each case is a recording
step and two reusing steps of one handle, Sigma scaled by 1e3 between the reusing steps, in the suite's NaN-filled workspace."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
# name: (n, me, mi), nb, group (panels per group; the lambda_i columns are the last mi)
SHAPES = {
    "lam_e_kept": ((256, 128, 1536), 128, 1),          # twelve lambda_i groups behind the kept lambda_e group
    "first_level": ((256, 0, 1536), 128, 1),           # no lambda_e: the first level alone
    "short_last_group": ((256, 256, 1408), 128, 2),    # groups of two panels, the last one a single panel
    # groups of five panels of 256 = 20 tiles: the hand-over into such a group is refused (more than 16 row tiles), the one into
    # the last group of two panels is split -- the fallback and the split in one step
    "refused_once": ((1280, 0, 3072), 256, 5),
    "nb256": ((512, 512, 1024), 256, 2),               # two lambda_i groups of 512 columns at nb = 256
}
FIRST = "lam_e_kept"


def _qp(shape):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=13)


def _vec(qp, k, variant=None):
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(4100 + k)
    v = dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
             ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=qp["s"] * rng.uniform(0.5, 2.0, mi),
             lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.3 / (k + 1))
    if k == 2:                          # Sigma = lambda_i / s scaled by 1e3 between the two reusing steps
        v["lda"][me:] *= 1.0e3
    if variant == "zero_lambda":        # lambda_i = 0 exactly on some rows: static pivots
        v["lda"][me + np.arange(5 + k, mi, 37)] = 0.0
    if variant == "flagged_tile":       # Sigma spread over 1e16 inside the 64 columns [64, 128)
        v["s"][64:128] *= 10.0 ** np.linspace(-8.0, 8.0, 64)
    return v


def _core(name, split, lookahead):
    from pyipm_amd.newton import NewtonCore
    shape, nb, group = SHAPES[name]
    env = {"PYIPM_TAIL_SPLIT": "1" if split else "0", "PYIPM_REUSE_X": "1"}
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
    core.set_option("tail_group", group)
    if lookahead is not None:
        core.set_option("lookahead", lookahead)
    return core


def _run(name, split, variant=None, lookahead=None, refine=0):
    """STEPS steps of one handle: [(dz bits, statistics)] and the bits of the factor storage's lower triangle behind the last one."""
    import torch
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    qp = _qp(SHAPES[name][0])
    core = _core(name, split, lookahead)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    out = []
    for k in range(STEPS):
        v = _vec(qp, k, variant)
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, refine)
        info = core.reuse_info()
        if lookahead != 0:              # (no lookahead: no reusable prefix, three full steps)
            assert info["reused"] == k and info["last"] == ("recording" if k == 0 else "reusing"), (name, k, info)
        out.append((dz.clone().view(torch.int64), st))
    store = core.kkt_storage()                                  # [column, row]
    lower = torch.triu(store.clone().view(torch.int64)).cpu()
    core.close()
    return out, lower


_REF = {}


def _ref(name, variant=None, lookahead=None, refine=0):
    """The old order (PYIPM_TAIL_SPLIT=0) on the same inputs: computed once per key, never changed."""
    import torch
    key = (name, variant, lookahead, refine)
    if key not in _REF:
        _REF[key] = _run(name, False, variant, lookahead, refine)
        dzs = [d.view(torch.float64) for d, _ in _REF[key][0]]
        for k in range(STEPS - 1):      # a stale value cannot hide: every entry of step k + 1 is another number
            assert bool((dzs[k + 1] != dzs[k]).all()), (name, k)
        assert all(bool(d.isfinite().all()) for d in dzs)
    return _REF[key]


def _same(got, ref, what):
    import torch
    for k in range(STEPS):
        assert torch.equal(got[0][k][0], ref[0][k][0]), (what, k)
        assert got[0][k][1] == ref[0][k][1], (what, k, got[0][k][1], ref[0][k][1])
    assert torch.equal(got[1], ref[1]), (what, "factor storage")


@pytest.mark.parametrize("name", list(SHAPES))
def test_same_bits_as_the_old_order(name):
    _same(_run(name, True), _ref(name), name)


def test_static_pivots():
    got, ref = _run(FIRST, True, "zero_lambda"), _ref(FIRST, "zero_lambda")
    assert all(st["n_zero"] > 0 for _, st in ref[0]), [st for _, st in ref[0]]
    _same(got, ref, "zero_lambda")


def test_a_flagged_tile():
    """Sigma spreads over 1e16 inside one 64-column tile: the tile is flagged and its columns take the refinement recurrence."""
    got, ref = _run(FIRST, True, "flagged_tile"), _ref(FIRST, "flagged_tile")
    _same(got, ref, "flagged_tile")
    assert all(st["d_max"] >= 1.0e12 * st["d_min"] for _, st in ref[0]), [st for _, st in ref[0]]


@pytest.mark.parametrize("lookahead", [0, 1, 2])
def test_lookahead(lookahead):
    _same(_run(FIRST, True, None, lookahead), _ref(FIRST, None, lookahead), ("lookahead", lookahead))


@pytest.mark.parametrize("refine", [0, 1])
def test_refine(refine):
    _same(_run("first_level", True, None, None, refine), _ref("first_level", None, None, refine), ("refine", refine))


_TRACE = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from pyipm_amd.newton import NewtonCore
from pyipm_amd.problems import make_qp
n, me, mi, nb, group = (int(a) for a in sys.argv[1:6])
qp = make_qp(n, me, mi, seed=13)
core = NewtonCore(n, me, mi, device=0, nb=nb)
core.set_option("expert", 1); core.set_option("group", group); core.set_option("tail_group", group)
core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
for k in range(2):
    core.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"] * (1.0 + k), qp["lam"], mu=qp["mu"])
    core.step(0.0, 0.0, 0)
    sys.stderr.write("---- step %%d %%s\n" %% (k, core.reuse_info()["last"]))
    sys.stderr.flush()
core.close()
"""
OLD = "head end (its first launch's stream) g%d"
# name: the least number of split hand-overs in a reusing step (lam_e_kept: eleven between its twelve lambda_i groups;
# first_level: the same behind the slack group; short_last_group: five between six groups; nb256: one between two groups;
# refused_once: exactly the last one, see below)
SPLITS = {"lam_e_kept": 11, "first_level": 11, "short_last_group": 5, "nb256": 1, "refused_once": 1}


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_split_is_planned_and_its_trace_marks_appear_in_the_stated_order(name):
    """PYIPM_GROUP_TRACE of a reusing step at every shape of this file: the hand-overs that SPLITS counts are split, each with
    "head begin", "diag head end", "rest of head end" and then the next group's "chain+rows begin", and without the old head's
    mark.  refused_once: the hand-over into the 20-tile group keeps the old head, the one behind it is split."""
    (n, me, mi), nb, group = SHAPES[name]
    env = dict(os.environ, PYIPM_GROUP_TRACE="1", PYIPM_TAIL_SPLIT="1", PYIPM_REUSE_X="1")
    pr = subprocess.run([sys.executable, "-c", _TRACE % ROOT] + [str(a) for a in (n, me, mi, nb, group)], env=env,
                        capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = pr.stderr
    assert "---- step 1 reusing" in text, text[-2000:]
    last = text[text.index("---- step 0"):text.index("---- step 1")]
    marks = [ln.split(" us ", 1)[1].strip() for ln in last.splitlines() if ln.startswith("[pyipm group trace]") and " us " in ln]
    split = [int(m.rsplit("g", 1)[1]) for m in marks if m.startswith("diag head end g")]
    assert len(split) >= SPLITS[name], marks
    for g in split:
        i = marks.index("diag head end g%d" % g)
        assert marks[i - 1] == "head begin g%d" % g, marks
        assert marks[i + 1] == "rest of head end g%d" % g, marks
        assert marks[i + 2] == "chain+rows begin g%d" % (g + 1), marks
        assert OLD % g not in marks, marks
    if name == "refused_once":
        assert len(split) == 1 and OLD % (split[0] - 1) in marks, marks
