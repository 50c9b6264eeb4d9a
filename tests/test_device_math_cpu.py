"""CPU: the polynomial sind / cosd / atan2d kernels of ekf_slam_amd/csrc/device_math.h (shared by the HIP kernels and the
host-side ekf_motion_model) against glibc, compiled for the host with g++."""
import subprocess

from helpers import host_build


def test_device_math_matches_libm(tmp_path):
    exe = host_build("host_math_check", str(tmp_path / "host_math_check"))
    out = subprocess.run([exe, "2000000"], check=True, capture_output=True, text=True).stdout.split()
    ms, mc, ma, ma2, bad = float(out[0]), float(out[1]), float(out[2]), float(out[3]), int(out[4])
    assert ms < 1.0 and mc < 1.0          # ulp
    assert ma < 2.0 and ma2 < 3.0         # atan2 includes the rounding of y / x
    assert bad == 0                       # zeros, infinities, NaN, exact values at multiples of 90 / 45 degrees
