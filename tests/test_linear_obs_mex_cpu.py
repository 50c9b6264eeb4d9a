"""CPU: the MEX gateway's `observe_linear` command under the MEX mock with a recording stand-in for ekf_observe_linear, the gateway
linked against a stand-in that lacks the symbol, and the MATLAB methods that forward to the command."""
import os
import re

from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_observe_linear(ekf_handle *h, const ekf_linear_obs *o, ekf_linear_result *res) {
    printf("ABI ekf_observe_linear z=%g,%g R=%g,%g,%g,%g Hr=%g,%g,%g,%g,%g,%g lm=%lld,%lld Hl0=%g,%g,%g,%g Hl1=%g,%g,%g,%g gate=%g wrap=%d,%d rows=%d wait=%d\n",
           o->z[0], o->z[1], o->R[0], o->R[1], o->R[2], o->R[3], o->Hr[0], o->Hr[1], o->Hr[2], o->Hr[3], o->Hr[4], o->Hr[5],
           (long long)o->lm[0], (long long)o->lm[1], o->Hl[0][0], o->Hl[0][1], o->Hl[0][2], o->Hl[0][3], o->Hl[1][0], o->Hl[1][1], o->Hl[1][2],
           o->Hl[1][3], o->gate, (int)o->wrap_deg[0], (int)o->wrap_deg[1], (int)o->rows, res != 0);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (res) { res->nu[0] = 0.5; res->nu[1] = -0.25; res->S[0] = 1; res->S[1] = 2; res->S[2] = 3; res->S[3] = 4; res->d2 = 1.5; res->outcome = EKF_LINEAR_GATED; }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *z = mock_double(2, 1, (const double[]){ 7, 8 }), *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *Hr = mock_double(2, 3, (const double[]){ 1, 2, 3, 4, 5, 6 }), *wrap = mock_double(2, 1, (const double[]){ 0, 1 });
    const mxArray *lm2 = mock_double(2, 1, (const double[]){ 5, 3 }), *Hl2 = mock_double(2, 4, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8 });
    const mxArray *none = mock_double(0, 0, 0);
    /* two landmarks [5 3] (1-based), no wait */
    const mxArray *two[11] = { mock_string("observe_linear"), h, z, R, Hr, lm2, Hl2, D1(9.5), wrap, D1(2), D1(0) };
    if (call("observe_linear", 1, 11, two)) return 1;
    /* a heading fix: no landmark, one row, the result waited for */
    const mxArray *head[11] = { mock_string("observe_linear"), h, mock_double(2, 1, (const double[]){ -179, 0 }), mock_double(2, 2, (const double[]){ 0.5, 0, 0, 0 }),
                                mock_double(2, 3, (const double[]){ 0, 0, 0, 0, 1, 0 }), none, none, D1(1.0 / 0.0), mock_double(2, 1, (const double[]){ 1, 0 }), D1(1), D1(1) };
    if (call("observe_linear heading", 1, 11, head)) return 1;
    const mxArray *bad[11];
    for (int q = 0; q < 11; ++q) bad[q] = two[q];
    if (!call("observe_linear", 1, 10, two)) return 1;
    bad[4] = mock_double(1, 5, (const double[]){ 1, 2, 3, 4, 5 });
    if (!call("observe_linear hr", 1, 11, bad)) return 1;
    bad[4] = Hr; bad[5] = mock_double(3, 1, (const double[]){ 1, 2, 3 }); bad[6] = mock_double(2, 6, 0);
    if (!call("observe_linear three", 1, 11, bad)) return 1;
    bad[5] = lm2; bad[6] = mock_double(2, 2, (const double[]){ 1, 0, 0, 1 });
    if (!call("observe_linear blocks", 1, 11, bad)) return 1;
    bad[5] = mock_double(2, 1, (const double[]){ 1.5, 2 }); bad[6] = Hl2;
    if (!call("observe_linear frac", 1, 11, bad)) return 1;
    bad[5] = lm2; bad[3] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("observe_linear badr", 1, 11, bad)) return 1;
    bad[3] = R; bad[1] = D1(1);
    if (!call("observe_linear noh", 1, 11, bad)) return 1;
    arm_failure();
    if (!call("observe_linear", 1, 11, two)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *ob[11] = { mock_string("observe_linear"), h, mock_double(2, 1, 0), mock_double(2, 2, 0), mock_double(2, 3, 0), mock_double(0, 0, 0),
                              mock_double(0, 0, 0), D1(1), mock_double(2, 1, 0), D1(2), D1(0) };
    if (!call("observe_linear", 1, 11, ob)) return 1;
''')


def test_mex_gateway_marshals_an_observation_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # MATLAB's lm = [5 3] arrives 0-based once, every block column-major as MATLAB holds it; no result asked for: an empty output
    i = t.index("ABI ekf_observe_linear z=7,8 R=4,1,1,9 Hr=1,2,3,4,5,6 lm=4,2 Hl0=1,2,3,4 Hl1=5,6,7,8 gate=9.5 wrap=0,1 rows=2 wait=0")
    assert t[i + 1] == "MEX observe_linear nrhs=11 -> ok out0=0x0[]"
    i = t.index("ABI ekf_observe_linear z=-179,0 R=0.5,0,0,0 Hr=0,0,0,0,1,0 lm=-1,-1 Hl0=0,0,0,0 Hl1=0,0,0,0 gate=inf wrap=1,0 rows=1 wait=1")
    assert t[i + 1] == "MEX observe_linear heading nrhs=11 -> ok out0=1x8[0.5,-0.25,1,2,3,4,1.5,2]"
    assert any(ln.startswith("MEX observe_linear nrhs=10 -> ERROR ekfslam:usage") and "needs 11 arguments" in ln for ln in t)
    for which, what in (("hr", "Hr needs 2 x 3 elements"), ("three", "at most two landmarks"), ("blocks", "one 2 x 2 block per landmark"),
                        ("frac", "whole numbers"), ("badr", "R needs 2 x 2 elements")):
        assert any(ln.startswith("MEX observe_linear %s nrhs=11 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX observe_linear noh nrhs=11 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_linear") for ln in t) == 3         # the two good calls and the injected failure
    assert "MEX observe_linear nrhs=11 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX observe_linear ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_observe_linear" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+res\s*=\s*observeLinear\(h,\s*z,\s*R,\s*Hr,\s*lm,\s*Hl,\s*gate,\s*wrap,\s*rows,\s*wait\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('observe_linear'," in m.group(1)
    for name, inner in (("fixLandmark", r"h\.observeLinear\(pos,\s*R,\s*\[\],\s*i,\s*eye\(2\)"), ("fixRobotPosition", r"h\.observeLinear\(pos,\s*R,\s*\[1 0 0; 0 1 0\]"),
                        ("fixRobotHeading", r"h\.observeLinear\(\[thetaDeg 0\],.*\[0 0 1; 0 0 0\],.*\[1 0\],\s*1,")):
        m = re.search(r"function\s+res\s*=\s*%s\((.*?)\n        end\b" % name, text, re.S)
        assert m and re.search(inner, m.group(1)), name
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "observe_linear")' in src and "#pragma weak ekf_observe_linear" in src
