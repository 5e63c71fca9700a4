"""Volume::DistanceField(grid, options, buffers) and Volume::ClassifyCells through the C++ class layer:
vulcan_amd/host/tests/distance_field_tests.cpp, run as test_gpu_merge_resample_host.py runs resample_tests."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vulcan_amd", "host", "bin")


@pytest.mark.gpu
def test_cpp_distance_field_tests_pass():
    exe = os.path.join(BIN, "distance_field_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(proc.stdout)
    assert proc.returncode == 0, proc.stdout[-4000:]
    assert re.search(r"3 test\(s\), 0 failed", proc.stdout)
    for name in ("DistanceField.ClearanceInFrontOfAWall", "DistanceField.AnEmptyVolumeIsUnknownAndFarFromAnything",
                 "DistanceField.AllowedWhileAFrameIsAnnounced"):
        assert f"[  OK  ] {name}" in proc.stdout
