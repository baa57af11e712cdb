"""slam-eds_amd/csrc/eds_splat.hpp, the sparse splat and blur the KLT and epiline kernels share, compiled for the host: every pixel's
merged sum equals a dense restatement of drawValuesPoints bit for bit (tests/cpp/splat_check.cpp; no GPU needed)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "splat_check.cpp")


def test_shared_splat_equals_dense_draw_values_points(tmp_path):
    exe = tmp_path / "splat_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", SRC, "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
