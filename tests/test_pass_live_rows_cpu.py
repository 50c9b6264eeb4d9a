"""CPU: the live-row bound of the in-place pass (PassJob::live_rows) on the kernel SOURCE of csrc/downdate.h, compiled for the host behind
tests/support/kernel_host_shim.h (tests/support/pass_live_rows_host_emulation.cpp says what the scene is): k_downdate_w -- plain, per-XCD
streams, with the row-panel extraction -- and k_downdate on a store of 3 x 3 tiles of edge 64 with 138 live rows.  The padding rows carry
sentinels and, beyond the slab that straddles the bound, a poisoned K: every sentinel has to survive, and the rows that hold state have to
equal the unbounded run bit for bit, in both walking directions and with a grid smaller than the item count."""
import subprocess

from helpers import host_build

CASES = ["k_downdate_w<double,64,8,false>", "k_downdate_w<double,64,16,false>", "k_downdate_w<double,64,64,false>",
         "k_downdate_w<double,64,8,true>", "k_downdate_w<double,64,32,true>", "k_downdate_w<double,64,8,false,+rowpanel>",
         "k_downdate<double,64,16>", "k_downdate<double,64,8>"]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == 4 * len(CASES) + 1
    for name in CASES:
        mine = [ln for ln in lines if ln.startswith(name + " reverse")]
        assert len(mine) == 4 and all(ln.endswith(": pass") and " sentinels 10368 moved 0," in ln for ln in mine), mine


def test_padding_rows_are_left_alone_and_live_rows_keep_their_bits(tmp_path):
    _run(host_build("pass_live_rows_host_emulation", str(tmp_path / "pass_live_rows")))


def test_the_same_program_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined: no lane reads or writes outside the store, the pair slots or the
    work lists, with and without the bound (nothing loaded into python is involved)."""
    _run(host_build("pass_live_rows_host_emulation", str(tmp_path / "pass_live_rows_san"),
                    flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
