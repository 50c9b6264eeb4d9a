"""CPU: the MEX gateway's `observe_model_joint_iterated` command under the MEX mock with a recording stand-in for
ekf_observe_model_joint_iterated, the gateway linked against a stand-in that lacks the symbol, and the MATLAB method that forwards to
the command."""
import os
import re

from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_observe_model_joint_iterated(ekf_handle *h, const ekf_model_obs *o, int64_t m, const int64_t *lm, double gate, int32_t iterations,
                                         double tol, ekf_joint_result *res, ekf_joint_iter_result *it, double *nu, double *S) {
    printf("ABI ekf_observe_model_joint_iterated m=%lld gate=%g iterations=%d tol=%g res=%d it=%d nu=%d S=%d\n", (long long)m, gate, (int)iterations,
           tol, res != 0, it != 0, nu != 0, S != 0);
    for (int64_t k = 0; k < m; ++k)
        printf("ABI   obs model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g -> %lld\n", (int)o[k].model, (int)o[k].reserved,
               o[k].z[0], o[k].z[1], o[k].R[0], o[k].R[1], o[k].R[2], o[k].R[3], (long long)o[k].lm[0], (long long)o[k].lm[1], o[k].anchor[0],
               o[k].anchor[1], o[k].gate, (long long)lm[k]);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    res->d2 = 0.25; res->dof = 3; res->pairings = 2; res->outcome = gate < 0.25 ? EKF_LINEAR_GATED : EKF_LINEAR_APPLIED; res->first_irregular = -1;
    it->used = gate < 0.25 ? 0 : iterations - 1; it->converged = gate < 0.25 ? 0 : 1; it->last_step = 0.5 * tol;
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    /* a scan of three (range and bearing (7, 8), a range 7.5, a relative position (1, 2)) paired with landmarks 2, none, 5 */
    const mxArray *model = mock_double(3, 1, (const double[]){ 1, 2, 4 }), *z = mock_double(3, 2, (const double[]){ 7, 7.5, 1, 8, 0, 2 });
    const mxArray *R = mock_double(4, 3, (const double[]){ 4, 1, 1, 9, 0.5, 0, 0, 0, 2, 0, 0, 3 }), *lm = mock_double(3, 1, (const double[]){ 2, 0, 5 });
    const mxArray *oj[9] = { mock_string("observe_model_joint_iterated"), h, model, z, R, lm, D1(11.5), D1(4), D1(0.125) };
    if (call("observe_model_joint_iterated", 1, 9, oj)) return 1;
    const mxArray *bad[9];
    for (int q = 0; q < 9; ++q) bad[q] = oj[q];
    bad[6] = D1(0.125);
    if (call("observe_model_joint_iterated gated", 1, 9, bad)) return 1;
    bad[6] = oj[6];
    if (!call("observe_model_joint_iterated", 1, 7, oj)) return 1;
    bad[2] = mock_double(33, 1, 0);
    if (!call("observe_model_joint_iterated many", 1, 9, bad)) return 1;
    bad[2] = model; bad[5] = mock_double(3, 1, (const double[]){ 1.5, 2, 3 });
    if (!call("observe_model_joint_iterated fraction", 1, 9, bad)) return 1;
    bad[5] = lm; bad[7] = D1(2.5);
    if (!call("observe_model_joint_iterated halfiter", 1, 9, bad)) return 1;
    bad[7] = D1(17);
    if (!call("observe_model_joint_iterated manyiter", 1, 9, bad)) return 1;
    bad[7] = D1(0);
    if (!call("observe_model_joint_iterated noiter", 1, 9, bad)) return 1;
    bad[7] = oj[7]; bad[8] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("observe_model_joint_iterated badtol", 1, 9, bad)) return 1;
    bad[8] = oj[8]; bad[1] = D1(1);
    if (!call("observe_model_joint_iterated noh", 1, 9, bad)) return 1;
    arm_failure();
    if (!call("observe_model_joint_iterated", 1, 9, oj)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *oj[9] = { mock_string("observe_model_joint_iterated"), h, D1(1), mock_double(1, 2, 0), mock_double(2, 2, 0), D1(1), D1(9), D1(3), D1(0) };
    if (!call("observe_model_joint_iterated", 1, 9, oj)) return 1;
''')


def test_mex_gateway_marshals_the_scan_and_the_controls_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_observe_model_joint_iterated m=3 gate=11.5 iterations=4 tol=0.125 res=1 it=1 nu=0 S=0")
    assert t[i + 1] == "ABI   obs model=1 reserved=0 z=7,8 R=4,1,1,9 lm=-1,-1 anchor=0,0 gate=inf -> 1"
    assert t[i + 2] == "ABI   obs model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=0,0 gate=inf -> -1"
    assert t[i + 3] == "ABI   obs model=4 reserved=0 z=1,2 R=2,0,0,3 lm=-1,-1 anchor=0,0 gate=inf -> 4"
    # d2 dof pairings outcome firstIrregular (1-based, 0 = none) used converged step
    assert t[i + 4] == "MEX observe_model_joint_iterated nrhs=9 -> ok out0=1x8[0.25,3,2,1,0,3,1,0.0625]"
    assert "MEX observe_model_joint_iterated gated nrhs=9 -> ok out0=1x8[0.25,3,2,2,0,0,0,0.0625]" in t
    assert any(ln.startswith("MEX observe_model_joint_iterated nrhs=7 -> ERROR ekfslam:usage") and "needs 9 arguments" in ln for ln in t)
    for which, what in (("many", "observe_model_joint_iterated: between 1 and 32 observations"), ("fraction", "landmark numbers (1-based)"),
                        ("halfiter", "iterations is a whole number, 1 .. 16"), ("manyiter", "iterations is a whole number, 1 .. 16"),
                        ("noiter", "iterations is a whole number, 1 .. 16"), ("badtol", "iterations and tol are one number each")):
        assert any(ln.startswith("MEX observe_model_joint_iterated %s nrhs=9 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX observe_model_joint_iterated noh nrhs=9 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_model_joint_iterated") for ln in t) == 3         # the two good calls and the injected failure
    assert "MEX observe_model_joint_iterated nrhs=9 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX observe_model_joint_iterated ") and "ERROR ekfslam:usage" in ln
               and "this libekfslam has no ekf_observe_model_joint_iterated" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+res\s*=\s*observeModelJointIterated\(h,\s*model,\s*z,\s*R,\s*lm,\s*gate,\s*iterations,\s*tol\)(.*?)\n        end\b", text, re.S)
    assert m and m.group(1).count("h.gateway('observe_model_joint_iterated', model, z, R, double(lm(:)), double(gate), double(iterations), double(tol))") == 1
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "observe_model_joint_iterated")' in src and "#pragma weak ekf_observe_model_joint_iterated" in src
    assert src.count("joint_scan(cmd, prhs, o, lm)") == 2                # one unpacking for both joint commands
