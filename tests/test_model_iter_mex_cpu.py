"""CPU: the MEX gateway's `observe_model_iterated` command under the MEX mock with a recording stand-in for ekf_observe_model_iterated,
the gateway linked against a stand-in that lacks the symbol, and the MATLAB method that forwards to the command."""
import os
import re

from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_observe_model_iterated(ekf_handle *h, const ekf_model_obs *o, int32_t iterations, double tol, ekf_linear_result *res, ekf_iterated_result *it) {
    printf("ABI ekf_observe_model_iterated model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g iterations=%d tol=%g first=%d it=%d\n",
           (int)o->model, (int)o->reserved, o->z[0], o->z[1], o->R[0], o->R[1], o->R[2], o->R[3], (long long)o->lm[0], (long long)o->lm[1], o->anchor[0],
           o->anchor[1], o->gate, (int)iterations, tol, res != 0, it != 0);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (res) { res->nu[0] = 0.5; res->nu[1] = -0.25; res->S[0] = 1; res->S[1] = 2; res->S[2] = 3; res->S[3] = 4; res->d2 = 1.5; res->outcome = EKF_LINEAR_APPLIED; }
    if (it) {
        it->S[0] = 5; it->S[1] = 6; it->S[2] = 7; it->S[3] = 8; it->nu[0] = 0.125; it->nu[1] = -0.5; it->used = 3; it->converged = 1; it->last_step = 0.0625;
        for (int k = 0; k < 7; ++k) it->x_local[k] = 10 + k;
    }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *z = mock_double(2, 1, (const double[]){ 7, 8 }), *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *lm1 = D1(5), *lm2 = mock_double(2, 1, (const double[]){ 5, 3 }), *none = mock_double(0, 0, 0);
    const mxArray *anchor = mock_double(2, 1, (const double[]){ 10, -4 });
    /* (h, model, z, R, lm, anchor, gate, iterations, tol, wait): range and bearing to landmark 5 (1-based), 8 linearisations, no wait */
    const mxArray *rb[11] = { mock_string("observe_model_iterated"), h, D1(1), z, R, lm1, none, D1(9.5), D1(8), D1(0.25), D1(0) };
    if (call("observe_model_iterated", 1, 11, rb)) return 1;
    /* the range to an anchor, the result waited for */
    const mxArray *an[11] = { mock_string("observe_model_iterated"), h, D1(2), mock_double(2, 1, (const double[]){ 7.5, 0 }),
                              mock_double(2, 2, (const double[]){ 0.5, 0, 0, 0 }), none, anchor, D1(1.0 / 0.0), D1(16), D1(0), D1(1) };
    if (call("observe_model_iterated anchor", 1, 11, an)) return 1;
    /* the distance between landmarks 5 and 3, one linearisation */
    const mxArray *lr[11] = { mock_string("observe_model_iterated"), h, D1(5), mock_double(2, 1, (const double[]){ 2.5, 0 }),
                              mock_double(2, 2, (const double[]){ 0.1, 0, 0, 0 }), lm2, none, D1(4), D1(1), D1(0), D1(0) };
    if (call("observe_model_iterated pair", 1, 11, lr)) return 1;
    const mxArray *bad[11];
    for (int q = 0; q < 11; ++q) bad[q] = rb[q];
    if (!call("observe_model_iterated", 1, 9, rb)) return 1;
    bad[5] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_model_iterated three", 1, 11, bad)) return 1;
    bad[5] = lm1; bad[6] = anchor;
    if (!call("observe_model_iterated both", 1, 11, bad)) return 1;
    bad[5] = none; bad[6] = none;
    if (!call("observe_model_iterated neither", 1, 11, bad)) return 1;
    bad[5] = D1(1.5);
    if (!call("observe_model_iterated frac", 1, 11, bad)) return 1;
    bad[5] = lm1; bad[4] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("observe_model_iterated badr", 1, 11, bad)) return 1;
    bad[4] = R; bad[3] = D1(1);
    if (!call("observe_model_iterated badz", 1, 11, bad)) return 1;
    bad[3] = z; bad[8] = D1(0);
    if (!call("observe_model_iterated zero", 1, 11, bad)) return 1;
    bad[8] = D1(17);
    if (!call("observe_model_iterated many", 1, 11, bad)) return 1;
    bad[8] = D1(2.5);
    if (!call("observe_model_iterated half", 1, 11, bad)) return 1;
    bad[8] = D1(8); bad[1] = D1(1);
    if (!call("observe_model_iterated noh", 1, 11, bad)) return 1;
    arm_failure();
    if (!call("observe_model_iterated", 1, 11, rb)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *ob[11] = { mock_string("observe_model_iterated"), h, D1(2), mock_double(2, 1, 0), mock_double(2, 2, 0), D1(1), mock_double(0, 0, 0), D1(1),
                              D1(3), D1(0), D1(0) };
    if (!call("observe_model_iterated", 1, 11, ob)) return 1;
''')


def test_mex_gateway_marshals_an_iterated_observation_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # the argument order (h, model, z, R, lm, anchor, gate, iterations, tol, wait); MATLAB's lm = 5 arrives 0-based once; no result asked
    # for: neither record is passed and the output is empty
    i = t.index("ABI ekf_observe_model_iterated model=1 reserved=0 z=7,8 R=4,1,1,9 lm=4,-1 anchor=0,0 gate=9.5 iterations=8 tol=0.25 first=0 it=0")
    assert t[i + 1] == "MEX observe_model_iterated nrhs=11 -> ok out0=0x0[]"
    i = t.index("ABI ekf_observe_model_iterated model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=10,-4 gate=inf iterations=16 tol=0 first=1 it=1")
    # observe_model's 8 values of the first linearisation, then S(:)' nu used converged lastStep xLocal
    assert t[i + 1] == ("MEX observe_model_iterated anchor nrhs=11 -> ok out0=1x24[0.5,-0.25,1,2,3,4,1.5,1,5,6,7,8,0.125,-0.5,3,1,0.0625,"
                        "10,11,12,13,14,15,16]")
    i = t.index("ABI ekf_observe_model_iterated model=5 reserved=0 z=2.5,0 R=0.1,0,0,0 lm=4,2 anchor=0,0 gate=4 iterations=1 tol=0 first=0 it=0")
    assert t[i + 1] == "MEX observe_model_iterated pair nrhs=11 -> ok out0=0x0[]"
    assert any(ln.startswith("MEX observe_model_iterated nrhs=9 -> ERROR ekfslam:usage") and "needs 11 arguments" in ln for ln in t)
    for which, what in (("three", "at most two landmarks"), ("both", "a landmark (anchor empty) or an anchor"), ("neither", "a landmark (anchor empty) or an anchor"),
                        ("frac", "whole numbers"), ("badr", "R needs 2 x 2 elements"), ("badz", "z needs 2 elements"),
                        ("zero", "iterations is a whole number, 1 .. 16"), ("many", "iterations is a whole number, 1 .. 16"),
                        ("half", "iterations is a whole number, 1 .. 16")):
        assert any(ln.startswith("MEX observe_model_iterated %s nrhs=11 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX observe_model_iterated noh nrhs=11 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_model_iterated") for ln in t) == 4          # the three good calls and the injected failure
    assert "MEX observe_model_iterated nrhs=11 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX observe_model_iterated ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_observe_model_iterated" in ln
               for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+res\s*=\s*observeModelIterated\(h,\s*model,\s*z,\s*R,\s*lm,\s*anchor,\s*gate,\s*iterations,\s*tol,\s*wait\)(.*?)\n        end\b",
                  text, re.S)
    assert m
    body = re.sub(r"\.\.\.[^\n]*\n\s*", "", m.group(1))
    assert ("h.gateway('observe_model_iterated', double(model), z, double(R), double(lm(:)), double(anchor(:)), double(gate), double(iterations), "
            "double(tol), double(wait))") in body
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "observe_model_iterated")' in src and "#pragma weak ekf_observe_model_iterated" in src
