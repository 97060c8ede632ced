"""The ring arithmetic of the pose, innovation and path histories (slam_amd/csrc/ring.h: slot, advance, check, stretches) against a
brute-force circular buffer, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/ring_check.cpp).
No GPU and no library needed: ring.h is plain C++."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_ring_against_brute_force_model_under_sanitizers(tmp_path):
    exe = tmp_path / "ring_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(HERE, "ring_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ring_check ok" in out.stdout
