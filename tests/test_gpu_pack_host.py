"""Volume::Pack, PackedVolume::Save / Load and Volume::Merge(pack) through the C++ class layer:
vulcan_amd/host/tests/pack_tests.cpp, run as test_gpu_merge_host.py runs merge_tests — and the map file the binary wrote,
read from Python: one format on both sides."""
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_support import api, sync  # noqa: F401
from vulcan_amd import io, vk_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vulcan_amd", "host", "bin")
NAMES = ("Pack.SavedAndLoadedRaycastsTheSame", "Pack.ABoxedPackHoldsTheBoxsBlocks", "Pack.NoBlocksNoCall",
         "Pack.MergeRefusedWhileAFrameIsAnnouncedPackAllowed")
W, H = 160, 120


def run(directory, *arguments):
    exe = os.path.join(BIN, "pack_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    proc = subprocess.run([exe, *arguments], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                          env=dict(os.environ, PACK_TESTS_DIR=str(directory)))
    print(proc.stdout)
    assert proc.returncode == 0, proc.stdout[-4000:]
    return proc.stdout


@pytest.mark.gpu
def test_cpp_pack_tests_pass(tmp_path):
    out = run(tmp_path)
    assert re.search(r"4 test\(s\), 0 failed", out)
    for name in NAMES:
        assert f"[  OK  ] {name}" in out


@pytest.mark.gpu
def test_python_loads_the_file_the_cpp_layer_wrote(api, tmp_path):
    """the map of pack_tests' slanted wall: the file as Python reads it, loaded into a volume of other table sizes and
    raycast from the pose the binary raycast from — the depth image the binary left"""
    out = run(tmp_path, "SavedAndLoaded")
    assert re.search(r"1 test\(s\), 0 failed", out)
    path = str(tmp_path / "pack_tests.map")
    origins, voxels, voxel_length, truncation_length = io.read_map(path)
    assert len(origins) > 500 and voxel_length == np.float32(0.008) and truncation_length == np.float32(0.04)
    assert os.path.getsize(path) == 32 + len(origins) * (8 + 10240)
    assert (voxels.view(T.voxel_dtype)["distance_weight"] == 2).sum() > 10000            # two integrations
    pack = api.PackedVolume.load(path)
    assert len(pack) == len(origins) and pack.host()[0].tobytes() == origins.tobytes()
    volume = api.Volume.load(path, 2039, 1024)
    # what Python packs of the loaded volume is the file's blocks
    again_origins, again_voxels = volume.pack().host()
    blocks = {tuple(o): voxels[10240 * k:10240 * (k + 1)].tobytes() for k, o in enumerate(origins)}
    assert {tuple(o): again_voxels[512 * k:512 * (k + 1)].tobytes() for k, o in enumerate(again_origins)} == blocks
    # SlantedFrame(Transform()) of volume_test_support.h, in float as the binary computes it
    y, x = np.mgrid[0:H, 0:W]
    depth = (np.float32(1.5) + np.float32(0.001) * x.astype(np.float32)) + np.float32(0.0007) * y.astype(np.float32)
    projection = T.Projection.make(136, 136, 80, 60)
    frame = api.Frame(depth.astype(np.float32), projection, T.Transform.identity())
    volume.set_view(frame, rounds=3)
    traced = api.Frame(np.zeros((H, W), np.float32), projection, T.Transform.identity())
    api.Tracer(volume).trace(traced)
    sync()
    want = np.fromfile(str(tmp_path / "pack_tests_depth.bin"), dtype=np.float32).reshape(H, W)
    got = traced.depth.cpu().numpy()
    print("pixels that differ:", int((got != want).sum()), "hits:", int((want > 0).sum()))
    assert (want > 0).sum() > W * H // 2
    assert got.tobytes() == want.tobytes()
