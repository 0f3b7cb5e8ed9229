"""The host rule of the L-BFGS pair store (pyipm_amd/csrc/pairs_rule.hpp: accept / skip / reset, the SS / L / D update) against
``pyipm_amd.loop.lbfgs_pair_update``, bit for bit: the same IEEE operations in the same order on the same products.
tests/pairs_rule_replay.cpp includes the header the library compiles and is built here with the host compiler and the address /
undefined-behaviour sanitizers; the products are NumPy's, carried as hexadecimal literals.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pairs_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZETA0 = 0.75
N = 37


def _hex(v):
    return float(v).hex()


def _numpy_run(memory, con, pattern):
    """IPM.lbfgs_update as it stands (NumPy storage, lbfgs_pair_update), recording the products of every offer and the state
    after it.  Returns (input text of the case, expected records)."""
    from pyipm_amd.loop import lbfgs_pair_update
    zeta, S, Y = ZETA0, np.zeros((N, 0)), np.zeros((N, 0))
    SS, L, D, fail = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)), 0
    seq = pc.offers(N, memory, pattern, pc.seed_of(N, memory, con, pattern))
    text = ["%d %d %s %s %d" % (memory, int(con), _hex(ZETA0), _hex(pc.EPS), len(seq))]
    want = []
    for x_old, x_new, g_old, g_new in seq:
        dx, dg = x_new - x_old, g_old[:N] - g_new[:N]
        drop = S.shape[1] > memory
        Sn = np.concatenate([S[:, 1:] if drop else S, dx[:, None]], axis=1)
        Yn = np.concatenate([Y[:, 1:] if drop else Y, dg[:, None]], axis=1)
        inner, cross = (Sn.T @ dx, dx @ Yn) if con else (Yn.T @ dg, Sn.T @ dg)
        curv, den = float(np.dot(dg, dx)), float(np.dot(dx, dx) if con else np.dot(dg, dg))
        text.append(" ".join([str(len(inner))] + [_hex(v) for v in inner] + [_hex(v) for v in cross] + [_hex(curv), _hex(den)]))
        accepted, reset, zeta, SS, L, D, fail = lbfgs_pair_update(zeta, SS, L, D, fail, drop, inner, cross, curv, den, con,
                                                                  memory, pc.EPS)
        if accepted:
            S, Y = Sn, Yn
        if reset:                                        # what lbfgs_init returns
            zeta, S, Y = ZETA0, np.zeros((N, 0)), np.zeros((N, 0))
            SS, L, D, fail = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)), 0
        want.append((2 if reset else int(accepted), S.shape[1], fail, zeta, SS.copy(), L.copy(), D.copy()))
    return "\n".join(text) + "\n", want


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pairs_rule") / "pairs_rule_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "pairs_rule_replay.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.parametrize("pattern", ["accepts", "reset", "empty"])
@pytest.mark.parametrize("memory", [1, 4, 31])
@pytest.mark.parametrize("con", [True, False])
def test_rule_is_lbfgs_pair_update_bit_for_bit(replay, con, memory, pattern):
    text, want = _numpy_run(memory, con, pattern)
    res = subprocess.run([replay], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(want) == 3 * (memory + 1) + 2
    outcomes = []
    for t, (line, (outcome, m, fail, zeta, SS, L, D)) in enumerate(zip(lines, want)):
        tok = line.split()
        assert (int(tok[0]), int(tok[1]), int(tok[2])) == (outcome, m, fail), (t, line[:80])
        got = np.array([float.fromhex(v) for v in tok[3:]])
        assert got.size == 1 + 3 * m * m
        assert got[0].tobytes() == np.float64(zeta).tobytes(), (t, got[0], zeta)
        for name, a, b in zip(("SS", "L", "D"), np.split(got[1:], 3), (SS, L, D)):
            assert a.tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes(), (t, name)
        outcomes.append(outcome)
    # what the case was built to meet did happen
    assert 0 in outcomes and 1 in outcomes
    assert max(w[1] for w in want) == memory + 1                      # the storage reached memory + 1 pairs and dropped
    if pattern == "reset":
        r = outcomes.index(2)
        assert want[r - 1][1] > 0 and want[r][1] == 0 and want[r][3] == ZETA0 and want[r + 1][1] == 1       # regrowth
    else:
        assert 2 not in outcomes                                       # "empty": memory + 1 skips on an empty store reset nothing
    if pattern == "empty":
        assert outcomes[:memory + 1] == [0] * (memory + 1) and want[memory][2] == memory + 1
