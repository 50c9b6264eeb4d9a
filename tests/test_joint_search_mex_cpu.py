"""CPU: the MEX gateway's `joint_search` command under the MEX mock with a recording stand-in for ekf_joint_search, the gateway linked
against a stand-in that lacks the symbol, and the MATLAB method that forwards to the command."""
import os
import re

from mex_harness import ROOT, driver, driver_without, prelude, transcript_of

_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_joint_search(ekf_handle *h, const ekf_model_obs *o, int64_t m, const double *threshold, int32_t beam, ekf_joint_search_result *res,
                         ekf_model_match *match, int64_t *cand, double *cand_d2, int64_t *alive_hyp, double *alive_d2) {
    printf("ABI ekf_joint_search m=%lld beam=%d match=%d cand=%d,%d alive=%d,%d\n", (long long)m, (int)beam, match != 0, cand != 0, cand_d2 != 0,
           alive_hyp != 0, alive_d2 != 0);
    for (int64_t k = 0; k < m; ++k)
        printf("ABI   obs model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g\n", (int)o[k].model, (int)o[k].reserved, o[k].z[0],
               o[k].z[1], o[k].R[0], o[k].R[1], o[k].R[2], o[k].R[3], (long long)o[k].lm[0], (long long)o[k].lm[1], o[k].anchor[0], o[k].anchor[1], o[k].gate);
    printf("ABI   threshold");
    for (int64_t d = 0; d <= 2 * m; ++d) printf(" %g", threshold[d]);
    printf("\n");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int k = 0; k < EKF_JOINT_MAX; ++k) { res->lm[k] = -1; res->tested[k] = res->survived[k] = 0; }
    res->lm[0] = 6; res->d2 = 0.25; res->dof = 2; res->pairings = 1; res->truncated = 1; res->nalive = 5; res->irregular = 3;
    for (int64_t k = 0; k < m; ++k) {
        match[k].best = k == 0 ? 6 : -1; match[k].second = -1; match[k].d2_best = k == 0 ? 0.5 : INFINITY; match[k].d2_second = INFINITY;
        match[k].within_gate = k == 0 ? 4 : 0; match[k].irregular = 0;
    }
    return EKF_OK;
}
'''

_SHOWN = prelude(r'''    for (int k = 0; k < nlhs && k < 3; ++k)
        if (out[k] && mxGetClassID(out[k]) != mxUINT64_CLASS) {
            printf(" out%d=%zux%zu[", k, mxGetM(out[k]), mxGetN(out[k]));
            for (size_t i = 0; i < mxGetM(out[k]) * mxGetN(out[k]); ++i) printf(i ? ",%g" : "%g", mxGetPr(out[k])[i]);
            printf("]");
        }
''')

_DRIVER = driver(r'''
    /* a scan of two: range and bearing (7, 8), a range 7.5; gate 9.21; thresholds for dof 0 .. 4; beam 8 */
    const mxArray *model = mock_double(2, 1, (const double[]){ 1, 2 }), *z = mock_double(2, 2, (const double[]){ 7, 7.5, 8, 0 });
    const mxArray *R = mock_double(4, 2, (const double[]){ 4, 1, 1, 9, 0.5, 0, 0, 0 }), *thr = mock_double(5, 1, (const double[]){ 0, 6.6, 9.2, 11.3, 13.3 });
    const mxArray *js[8] = { mock_string("joint_search"), h, model, z, R, D1(9.21), thr, D1(8) };
    if (call("joint_search", 1, 8, js)) return 1;
    if (call("joint_search all", 3, 8, js)) return 1;
    const mxArray *bad[8];
    for (int q = 0; q < 8; ++q) bad[q] = js[q];
    if (!call("joint_search", 1, 7, js)) return 1;
    bad[2] = mock_double(0, 0, 0);
    if (!call("joint_search none", 1, 8, bad)) return 1;
    bad[2] = mock_double(33, 1, 0);
    if (!call("joint_search many", 1, 8, bad)) return 1;
    bad[2] = model; bad[3] = mock_double(2, 1, (const double[]){ 7, 8 });
    if (!call("joint_search badz", 1, 8, bad)) return 1;
    bad[3] = z; bad[4] = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    if (!call("joint_search badr", 1, 8, bad)) return 1;
    bad[4] = R; bad[5] = mock_double(2, 1, (const double[]){ 9, 9 });
    if (!call("joint_search badgate", 1, 8, bad)) return 1;
    bad[5] = js[5]; bad[6] = mock_double(4, 1, (const double[]){ 0, 1, 2, 3 });
    if (!call("joint_search badthr", 1, 8, bad)) return 1;
    bad[6] = thr; bad[7] = D1(65);
    if (!call("joint_search bigbeam", 1, 8, bad)) return 1;
    bad[7] = D1(2.5);
    if (!call("joint_search fraction", 1, 8, bad)) return 1;
    bad[7] = js[7]; bad[1] = D1(1);
    if (!call("joint_search noh", 1, 8, bad)) return 1;
    arm_failure();
    if (!call("joint_search", 1, 8, js)) return 1;
''', _SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *js[8] = { mock_string("joint_search"), h, D1(1), mock_double(1, 2, 0), mock_double(2, 2, 0), D1(9), mock_double(3, 1, 0), D1(8) };
    if (!call("joint_search", 1, 8, js)) return 1;
''')


def test_mex_gateway_marshals_the_scan_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # every entry searches: lm = {-1, -1}, the anchor zero, the candidate gate on every entry; the match records always asked for
    i = t.index("ABI ekf_joint_search m=2 beam=8 match=1 cand=0,0 alive=0,0")
    assert t[i + 1] == "ABI   obs model=1 reserved=0 z=7,8 R=4,1,1,9 lm=-1,-1 anchor=0,0 gate=9.21"
    assert t[i + 2] == "ABI   obs model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=0,0 gate=9.21"
    assert t[i + 3] == "ABI   threshold 0 6.6 9.2 11.3 13.3"
    head = "out0=1x6[0.25,2,1,1,5,3]"
    assert t[i + 4] == "MEX joint_search nrhs=8 -> ok " + head
    # the winner 1-based with 0 = left out; per entry [withinGate best d2Best], best 1-based with 0 = none
    assert "MEX joint_search all nrhs=8 -> ok " + head + " out1=2x1[7,0] out2=2x3[4,0,7,0,0.5,inf]" in t
    assert any(ln.startswith("MEX joint_search nrhs=7 -> ERROR ekfslam:usage") and "needs 8 arguments" in ln for ln in t)
    for which, what in (("none", "between 1 and 32 observations"), ("many", "between 1 and 32 observations"), ("badz", "z needs m x 2 elements"),
                        ("badr", "R needs 2 x 2 x m elements"), ("badgate", "gate is one number"), ("badthr", "threshold needs 2 m + 1 elements"),
                        ("bigbeam", "whole number between 1 and 64"), ("fraction", "whole number between 1 and 64")):
        assert any(ln.startswith("MEX joint_search %s nrhs=8 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX joint_search noh nrhs=8 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_joint_search") for ln in t) == 3             # the two good calls and the injected failure
    assert "MEX joint_search nrhs=8 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX joint_search ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_joint_search" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[res,\s*lm,\s*match\]\s*=\s*jointSearch\(h,\s*model,\s*z,\s*R,\s*gate,\s*threshold,\s*beam\)(.*?)\n        end\b", text, re.S)
    assert m and m.group(1).count("h.gateway('joint_search', model, z, R, double(gate), double(threshold(:)), double(beam))") == 1
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "joint_search")' in src and "#pragma weak ekf_joint_search" in src
