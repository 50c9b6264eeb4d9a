"""CPU: the three search kernels of ekf_joint_search (k_joint_search_prepare / _extend / _select of ekf_slam_amd/csrc/joint_search.h)
compiled for the host and run on the emulated state by tests/support/joint_search_host_emulation.cpp -- tile edge 16, N = 41 (a padded
tail, the cluster ending in the last landmark) and 150, F64 and float stores, 0 and 3 pending pairs -- on the 2-entry scene, the clusters
K = 4, 6, 8 at beams 64 and 2 and the mixed scan.  The program itself compares every alive hypothesis bit for bit with k_joint_innovation
(joint_phases) emulated on the same state and checks that every buffer of the state is unchanged; here its answers stand against the NumPy
level loop of tests/joint_search_cases.py on the dense state the program reports.  No GPU."""
import math
import subprocess

import numpy as np
import pytest

import joint_cases as J
import joint_search_cases as S
import model_obs_cases as M
from helpers import host_build

RTOL_D2 = 1e-9                        # tests/test_joint_cpu.py's tolerance of a joint d2 against joint_dense


def chi2_any(p, dof):
    """chi2_table for every dof: bisection on the regularised incomplete gamma function through math.erf / the even series."""
    if dof % 2 == 0:
        return J.chi2_table(p, dof)
    def cdf(q):                                               # odd dof: erf(sqrt(q / 2)) minus the half-integer series
        t = math.erf(math.sqrt(q / 2.0))
        term = math.sqrt(2.0 * q / math.pi) * math.exp(-q / 2.0)
        for j in range(1, dof, 2):
            t -= term
            term *= q / (j + 2.0)
        return t
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def scene(name, N):
    """(x, P, entries) of a scene on N landmarks; with N = 41 the cluster ends in landmark 40, alone in its padded tile row."""
    if name == "two" and N == S.N0:
        x, _, d, U, scan = J.ambiguous_scene()
        return x, np.diag(d) + U @ U.T, J.scene_entries(scan, S.GATE)
    K = {"two": 2, "mixed": 4}.get(name) or int(name[1:])
    lm0 = S.LM0 if N == S.N0 else N - K
    x, _, d, U, scan = S.cluster_scene(K, N, lm0)
    return x, np.diag(d) + U @ U.T, (S.mixed_scan(x, lm0) if name == "mixed" else J.scene_entries(scan, S.GATE))


# (scene, beam) on N = 150 / F64 / nothing pending and on N = 41 / float / 3 pending; the other two corners on K4 and the mixed scan
CASES = [(name, beam, N, f32, pend) for name in ("two", "K4", "K6", "K8", "mixed") for beam in (64, 2)
         for N, f32, pend in ((150, 0, 0), (41, 1, 3))] + \
        [(name, 64, N, f32, pend) for name in ("K4", "mixed") for N, f32, pend in ((150, 1, 3), (41, 0, 0), (150, 0, 3), (41, 1, 0))]


def parsed_R(ent):
    """R as the library parses it: row-major 2 x 2, a one-row model [r, 0, 0, 1]."""
    if M.ROWS[ent["model"]] == 2:
        return np.asarray(ent["R"], dtype=np.float64).reshape(-1)
    return np.array([float(np.asarray(ent["R"]).reshape(-1)[0]), 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    d = tmp_path_factory.mktemp("joint_search_emulation")
    exe = host_build("joint_search_host_emulation", str(d / "joint_search_host_emulation"))
    blocks, given = [np.array([float(len(CASES))])], []
    for name, beam, N, f32, pend in CASES:
        x, P, ents = scene(name, N)
        thr = [chi2_any(S.JOINT_P, dof) for dof in range(2 * len(ents) + 1)]
        given.append((ents, thr))
        blocks += [np.array([N, len(ents), beam, pend, f32], dtype=np.float64), x, P.reshape(-1)]
        for en in ents:
            z = np.zeros(2)
            z[:M.ROWS[en["model"]]] = en["z"]
            blocks.append(np.concatenate([[en["model"]], z, parsed_R(en), [en["gate"]]]))
        blocks.append(np.array(thr))
    np.concatenate(blocks).astype(np.float64).tofile(d / "cases.bin")
    r = subprocess.run([exe, str(d / "cases.bin"), str(d / "out.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    raw, pos, out = np.fromfile(d / "out.bin", dtype=np.float64), 0, []
    for ents, thr in given:
        n, m = int(raw[pos]), int(raw[pos + 1]); pos += 2
        assert m == len(ents)
        x = raw[pos:pos + n]; pos += n
        P = raw[pos:pos + n * n].reshape(n, n); pos += n * n
        lm = raw[pos:pos + m].astype(np.int64); pos += m
        d2, dof, pairings, truncated, nalive, irregular = raw[pos:pos + 6]; pos += 6
        tested = raw[pos:pos + m].astype(np.int64); pos += m
        survived = raw[pos:pos + m].astype(np.int64); pos += m
        alive_d2 = raw[pos:pos + 64]; pos += 64
        bad = int(raw[pos]); pos += 1
        out.append(dict(x=x, P=P, ents=ents, thr=thr, landmark=lm, d2=d2, dof=int(dof), pairings=int(pairings), truncated=bool(truncated),
                        nalive=int(nalive), irregular=int(irregular), tested=tested, survived=survived, alive_d2=alive_d2, bad=bad))
    assert pos == raw.size
    return out


@pytest.mark.parametrize("index", range(len(CASES)), ids=["%s-beam%d-N%d-%s-%dpending" % (c[0], c[1], c[2], "f32" if c[3] else "f64", c[4]) for c in CASES])
def test_the_emulated_kernels_against_the_numpy_level_loop(emulated, index):
    name, beam, N, f32, pend = CASES[index]
    got = emulated[index]
    assert got["bad"] == 0                                    # bit for bit against joint_phases; every buffer unchanged; the lists as given
    margin = []
    want = S.numpy_search(got["x"], got["P"], got["ents"], got["thr"], beam, margin)
    assert not margin or min(margin) > 1e-9, "an extension lies on its threshold: the comparison of the counters would be a coin toss"
    for key in ("landmark", "tested", "survived"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["truncated"], got["nalive"], got["dof"], got["pairings"]) == (want["truncated"], want["nalive"], want["dof"], want["pairings"])
    np.testing.assert_allclose(got["d2"], want["d2"], rtol=RTOL_D2)
    np.testing.assert_allclose(got["alive_d2"][:got["nalive"]], want["alive_d2"], rtol=RTOL_D2)
    assert np.all(np.isnan(got["alive_d2"][got["nalive"]:])) and got["irregular"] == want["irregular"]
    if name == "mixed":
        assert got["tested"][1] == 0 and got["survived"][1] == 0 and got["landmark"][1] == -1
    if name.startswith("K") and (N, f32, pend) == (150, 0, 0):                  # the scene of the premises, on the kernels
        ref = S.cluster_reference(int(name[1:]), beam)[4]
        for key in ("landmark", "tested", "survived"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
