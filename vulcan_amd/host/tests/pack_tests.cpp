// pack_tests.cpp — Volume::Pack, PackedVolume::Save / Load and Volume::Merge(pack) through the C++ class layer -> C ABI ->
// HIP kernels (no upstream case: the reference's Volume is a process-wide singleton that never leaves its buffers,
// src/volume.cu:17-21). The calls' exact outcome is held against their CPU statement by tests/test_gpu_pack.py; these
// cases are what a user of the classes sees: a map written to a file and read back into a volume of other table sizes
// raycasts to the same image, a boxed pack holds the box's blocks, a pack without blocks costs no call, and Merge(pack)
// refuses to run on top of an announced frame while Pack does not. Harness: volume_test_support.h.
//
//   ./pack_tests            run everything (needs a GPU)
//   ./pack_tests <filter>   run the cases whose name contains <filter>
// With PACK_TESTS_DIR set, SavedAndLoadedRaycastsTheSame leaves pack_tests.map and the raycast's depth image
// (pack_tests_depth.bin, 160 x 120 floats) there: tests/test_gpu_pack_host.py reads both from Python.
#include <cstdlib>

#include "volume_test_support.h"

static std::string Directory()
{
  for (const char* name : {"PACK_TESTS_DIR", "TMPDIR"})
    if (const char* value = std::getenv(name))
      if (*value) return value;
  return "/tmp";
}

static std::vector<float> Raycast(const std::shared_ptr<Volume>& volume, const Frame& frame)
{
  volume->SetView(frame, 3);
  Frame traced;
  traced.depth_to_world_transform = frame.depth_to_world_transform;
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(volume);
  tracer.Trace(traced);
  std::vector<float> depth(traced.depth_image->GetTotal());
  traced.depth_image->CopyToHost(depth.data());
  Device::Synchronize();
  return depth;
}

static BlockMap Blocks(const std::vector<int16_t>& origins, const std::vector<vk_voxel>& voxels)
{
  BlockMap out;
  for (size_t k = 0; k < origins.size() / 4; ++k)
    out[{{origins[4 * k], origins[4 * k + 1], origins[4 * k + 2]}}] = voxels.data() + k * VK_BLOCK_VOXELS;
  return out;
}

struct HostPack
{
  std::vector<int16_t> origins;
  std::vector<vk_voxel> voxels;
};

static HostPack Download(const PackedVolume& pack)
{
  HostPack host;
  host.origins.resize(size_t(pack.Count()) * 4);
  host.voxels.resize(size_t(pack.Count()) * VK_BLOCK_VOXELS);
  if (pack.Count() > 0)
  {
    pack.GetOrigins().CopyToHost(host.origins.data());
    VK_ASSERT(vk_memcpy_d2h(host.voxels.data(), pack.GetVoxels().GetData(), pack.GetVoxels().GetSize(), Device::GetStream()));
    Device::Synchronize();
  }
  return host;
}

// a map packed, saved, loaded into a fresh volume of other table sizes, raycast from the same pose: the same depth image
TEST(Pack, SavedAndLoadedRaycastsTheSame)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);          // long chains
  // a bucket takes one block a round: let the view settle, so that the SetView calls in front of the raycasts below
  // allocate nothing in either volume (the blocks that arrive here are in the map, unobserved, and travel with it)
  for (int i = 0; i < 2; ++i) volume->SetView(frame, 8);
  const int blocks = volume->GetAllocatedBlockCount();
  ASSERT_TRUE(blocks > 500);
  const PackedVolume pack = volume->Pack();
  ASSERT_EQ(blocks, pack.Count());
  ASSERT_EQ(size_t(blocks) * 4, pack.GetOrigins().GetSize());
  ASSERT_EQ(size_t(blocks) * 10240, pack.GetVoxels().GetSize());
  ASSERT_TRUE(pack.VoxelLength() == kVoxel && pack.TruncationLength() == volume->GetTruncationLength());
  ASSERT_EQ(blocks, volume->GetAllocatedBlockCount());              // the volume is only read

  // the pack holds the volume's blocks, in the order of the table's entries
  const std::vector<vk_hash_entry> entries = Entries(*volume);
  const std::vector<vk_voxel> voxels = Voxels(*volume);
  const HostPack host = Download(pack);
  size_t k = 0;
  for (const vk_hash_entry& e : entries)
  {
    if (e.data < 0) continue;
    ASSERT_TRUE(k < size_t(blocks));
    for (int a = 0; a < 3; ++a) ASSERT_EQ(e.block.origin[a], host.origins[4 * k + a]);
    ASSERT_EQ(0, host.origins[4 * k + 3]);
    ASSERT_TRUE(std::memcmp(voxels.data() + size_t(e.data) * VK_BLOCK_VOXELS, host.voxels.data() + k * VK_BLOCK_VOXELS, 10240) == 0);
    ++k;
  }
  ASSERT_EQ(size_t(blocks), k);

  const std::string path = Directory() + "/pack_tests.map";
  pack.Save(path);
  const PackedVolume read = PackedVolume::Load(path);
  ASSERT_EQ(blocks, read.Count());
  ASSERT_TRUE(read.VoxelLength() == pack.VoxelLength() && read.TruncationLength() == pack.TruncationLength());
  const HostPack again = Download(read);
  ASSERT_TRUE(again.origins == host.origins);
  ASSERT_TRUE(std::memcmp(again.voxels.data(), host.voxels.data(), size_t(blocks) * 10240) == 0);

  auto loaded = Volume::Load(path, 1021, 2048);                    // other table sizes
  ASSERT_EQ(blocks, loaded->GetAllocatedBlockCount());
  ASSERT_TRUE(loaded->GetVoxelLength() == kVoxel);
  const std::vector<vk_hash_entry> entries_l = Entries(*loaded);
  const std::vector<vk_voxel> voxels_l = Voxels(*loaded);
  const BlockMap want = Blocks(entries, voxels), got = Blocks(entries_l, voxels_l);
  ASSERT_EQ(want.size(), got.size());
  for (const auto& block : want)
  {
    ASSERT_TRUE(got.count(block.first) == 1);
    ASSERT_TRUE(std::memcmp(block.second, got.at(block.first), sizeof(vk_voxel) * VK_BLOCK_VOXELS) == 0);
  }

  const std::vector<float> depth = Raycast(volume, frame), depth_loaded = Raycast(loaded, frame);
  ASSERT_EQ(blocks, volume->GetAllocatedBlockCount());              // the view had settled
  ASSERT_EQ(blocks, loaded->GetAllocatedBlockCount());
  int hits = 0;
  for (float d : depth) hits += d > 0.0f ? 1 : 0;
  ASSERT_TRUE(hits > kWidth * kHeight / 2);
  ASSERT_TRUE(std::memcmp(depth.data(), depth_loaded.data(), depth.size() * sizeof(float)) == 0);

  if (std::getenv("PACK_TESTS_DIR"))
  {
    std::FILE* file = std::fopen((Directory() + "/pack_tests_depth.bin").c_str(), "wb");
    ASSERT_TRUE(file != nullptr);
    ASSERT_EQ(depth.size(), std::fwrite(depth.data(), sizeof(float), depth.size(), file));
    std::fclose(file);
  }
  else std::remove(path.c_str());

  // a file that is not a map is refused before anything reaches the device
  const std::string bad = Directory() + "/pack_tests_bad.map";
  std::FILE* file = std::fopen(bad.c_str(), "wb");
  ASSERT_TRUE(file != nullptr);
  std::fputs("VULCANMP, but nothing else of a map file is here", file);
  std::fclose(file);
  ASSERT_THROW(PackedVolume::Load(bad));
  std::remove(bad.c_str());
}

// a boxed pack holds the blocks inside the box and no other; merged into a fresh volume they are what arrives
TEST(Pack, ABoxedPackHoldsTheBoxsBlocks)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 2);
  const std::vector<vk_hash_entry> entries = Entries(*volume);
  const std::vector<vk_voxel> voxels = Voxels(*volume);
  const BlockMap all = Blocks(entries, voxels);
  // the box: around the mean origin, half the extent either way
  long sum[3] = {0, 0, 0};
  for (const auto& block : all) for (int a = 0; a < 3; ++a) sum[a] += block.first[a];
  PackOptions options;
  options.box = true;
  for (int a = 0; a < 3; ++a)
  {
    const int mean = int(sum[a] / long(all.size()));
    options.lo[a] = int16_t(mean - 3);
    options.hi[a] = int16_t(mean + 3);
  }
  size_t inside = 0;
  for (const auto& block : all)
  {
    bool in = true;
    for (int a = 0; a < 3; ++a) in = in && block.first[a] >= options.lo[a] && block.first[a] <= options.hi[a];
    inside += in ? 1 : 0;
  }
  ASSERT_TRUE(inside > 10 && inside < all.size());
  const PackedVolume pack = volume->Pack(options);
  ASSERT_EQ(inside, size_t(pack.Count()));
  const HostPack host = Download(pack);
  const BlockMap packed = Blocks(host.origins, host.voxels);
  ASSERT_EQ(inside, packed.size());                                 // distinct origins
  for (const auto& block : packed)
  {
    for (int a = 0; a < 3; ++a) ASSERT_TRUE(block.first[a] >= options.lo[a] && block.first[a] <= options.hi[a]);
    ASSERT_TRUE(all.count(block.first) == 1);
    ASSERT_TRUE(std::memcmp(block.second, all.at(block.first), sizeof(vk_voxel) * VK_BLOCK_VOXELS) == 0);
  }
  // skip_unobserved on top: no more blocks, and every one has a weight somewhere
  options.skip_unobserved = true;
  const PackedVolume observed = volume->Pack(options);
  ASSERT_TRUE(observed.Count() > 0 && observed.Count() <= pack.Count());
  const HostPack seen = Download(observed);
  for (int k = 0; k < observed.Count(); ++k)
  {
    bool any = false;
    for (int i = 0; i < VK_BLOCK_VOXELS; ++i)
      any = any || seen.voxels[size_t(k) * VK_BLOCK_VOXELS + i].distance_weight != 0 || seen.voxels[size_t(k) * VK_BLOCK_VOXELS + i].color_weight != 0;
    ASSERT_TRUE(any);
  }
  // into a fresh volume: the box's blocks and nothing else
  auto fresh = Fresh(1021, 2048);
  MergeOptions caps;
  caps.max_distance_weight = caps.max_color_weight = 32767.0f;
  const MergeCounts counts = fresh->Merge(pack, caps);
  ASSERT_EQ(inside, size_t(counts.considered));
  ASSERT_EQ(inside, size_t(counts.fused));
  ASSERT_EQ(inside, size_t(counts.allocated));
  ASSERT_EQ(0, counts.left_out);
  ASSERT_EQ(int(inside), fresh->GetAllocatedBlockCount());
  // a box the wrong way round is refused
  options.lo[0] = 5;
  options.hi[0] = 4;
  ASSERT_THROW(volume->Pack(options));
}

// no blocks: the pack is empty, and merging it makes no call
TEST(Pack, NoBlocksNoCall)
{
  auto empty = Fresh(61, 7);
  const PackedVolume pack = empty->Pack();
  ASSERT_EQ(0, pack.Count());
  ASSERT_EQ(size_t(0), pack.GetVoxels().GetSize());
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  volume->SetView(frame);
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 100);
  const int blocks = volume->GetAllocatedBlockCount();
  const MergeCounts counts = volume->Merge(pack);
  ASSERT_EQ(0, counts.considered);
  ASSERT_EQ(0, counts.fused);
  ASSERT_EQ(0, counts.rounds);
  ASSERT_EQ(blocks, volume->GetAllocatedBlockCount());
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());         // no call: the visible list is still the SetView's
  // a box that holds nothing
  PackOptions options;
  options.box = true;
  for (int a = 0; a < 3; ++a) options.lo[a] = options.hi[a] = 3000;
  ASSERT_EQ(0, volume->Pack(options).Count());
  // an empty pack goes through a file as well
  const std::string path = Directory() + "/pack_tests_empty.map";
  pack.Save(path);
  ASSERT_EQ(0, PackedVolume::Load(path).Count());
  std::remove(path.c_str());
  // and a pack of another lattice is refused
  auto coarse = std::make_shared<Volume>(509, 64);
  coarse->SetVoxelLength(0.016f);
  ASSERT_THROW(coarse->Merge(volume->Pack()));
}

// Merge(pack) between SetView calls only; Pack only reads and is allowed while a frame is announced
TEST(Pack, MergeRefusedWhileAFrameIsAnnouncedPackAllowed)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  auto other = Fused(8192, 2048, SlantedFrame(Transform::Translate(0.3f, 0.0f, 0.0f)), 1);
  const PackedVolume pack = other->Pack();
  ASSERT_EQ(other->GetAllocatedBlockCount(), pack.Count());
  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = SlantedFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int before = volume->GetAllocatedBlockCount();
  ASSERT_THROW(volume->Merge(pack));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  const PackedVolume held = volume->Pack();                         // allowed: the volume is only read
  ASSERT_EQ(before, held.Count());
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  volume->CancelRequestsAhead(3);
  const int announced = volume->GetAllocatedBlockCount();
  const MergeCounts counts = volume->Merge(pack);
  ASSERT_EQ(pack.Count(), counts.fused);
  ASSERT_EQ(announced + counts.allocated, volume->GetAllocatedBlockCount());
}

int main(int argc, char** argv) { return RunTests("pack_tests", argc, argv); }
