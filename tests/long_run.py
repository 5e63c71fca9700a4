"""The long run's parity leg, shared by tools/soak.py and tests/test_gpu_long_run.py: the room sequence at the bench's size
(tests/golden/make_fixtures.py soak_inputs: 240 distinct frames, one swing of the camera) resident on the device, looped to
any length, and the digests of a bench.FrameLoop's state that tests/golden/soak_room_640x480.json holds for the oracle.
Imports nothing of the device until it is called."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.join(HERE, "golden")):
    if path not in sys.path:
        sys.path.insert(0, path)

DIGEST_KEYS = ("entries_sha256", "voxels_sha256", "depth_sha256", "color_sha256", "normals_sha256", "visible", "voxel_pointer",
               "dropped")


class Looped:
    """a list that repeats: frame i of the run is frame i mod 240 of the room sequence"""

    def __init__(self, items, length):
        self.items, self.length = items, length

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        return self.items[i % len(self.items)]


def resident_room(inputs):
    """a bench.RoomSequence around [(depth, colour, pose)] (make_fixtures.soak_inputs): the images on the device"""
    import torch
    import bench
    room = bench.RoomSequence.__new__(bench.RoomSequence)
    room.truth = [p for _, _, p in inputs]
    room.depth = [torch.from_numpy(d).cuda() for d, _, _ in inputs]
    room.color = [torch.from_numpy(c).cuda() for _, c, _ in inputs]
    torch.cuda.synchronize()
    return room


def looped(room, n):
    """`n` frames of `room`, over and over (the same resident images)"""
    import bench
    seq = bench.RoomSequence.__new__(bench.RoomSequence)
    seq.truth, seq.depth, seq.color = Looped(room.truth, n), Looped(room.depth, n), Looped(room.color, n)
    return seq


def digests(loop):
    """what a checkpoint of tests/golden/soak_room_640x480.json holds (make_fixtures.soak_oracle), of a bench.FrameLoop
    behind its last step: the hash table, every voxel byte, the raycast images — hashed by make_fixtures.digest, as the
    oracle's were — the visible count, the free-slot pointer and the dropped requests"""
    import torch
    import make_fixtures as mf
    from vulcan_amd import vk_types as T
    torch.cuda.synchronize()
    vol = loop.vols[0]["vol"]
    ctr = vol.read_counters()
    images = {"entries_sha256": vol.hash_entries, "voxels_sha256": vol.voxels, "depth_sha256": loop.key.depth,
              "color_sha256": loop.key.color, "normals_sha256": loop.key.normals}
    got = {key: mf.digest(t.cpu().numpy()) for key, t in images.items()}
    got.update(visible=int(ctr[T.VK_CTR_VISIBLE]), voxel_pointer=int(ctr[T.VK_CTR_VOXEL_PTR]), dropped=int(ctr[T.VK_CTR_DROPPED]))
    assert sorted(got) == sorted(DIGEST_KEYS)
    return got
