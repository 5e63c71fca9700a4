// resample_tests.cpp — Volume::MergeResampled(other, Tdst_src, supersample) through the C++ class layer -> C ABI -> HIP
// kernels (no upstream case: the reference's Volume is a process-wide singleton, src/volume.cu:17-21). The call's exact
// outcome is held against its CPU statement by tests/test_gpu_merge_resample.py; these cases are what a user of the class
// sees: a copy of a fused map at twice the voxel length raycasts as the surface the map was fused from, at equal lengths
// and one sample point the call is Merge(other, Tdst_src), and it is refused while a frame is announced. Harness:
// volume_test_support.h.
//
//   ./resample_tests            run everything (needs a GPU)
//   ./resample_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// a wall fused at 8 mm, copied into a fresh volume at 16 mm (two sample points per axis by default), seen from the camera
// that fused it: the raycast finds the wall where the depth image had it. The copy's field is a mean of samples of a field
// close to linear across the surface, so its zero crossing moves by a fraction of a coarse voxel: half of one bounds the mean.
TEST(Resample, ATwoToOneCopyRaycastsTheSameSurface)
{
  const Frame frame = SlantedFrame(Transform());
  auto source = Fused(8192, 2048, frame, 2);
  auto coarse = std::make_shared<Volume>(8192, 2048);
  coarse->SetVoxelLength(2.0f * kVoxel);
  const MergePoseCounts counts = coarse->MergeResampled(*source, Transform());
  ASSERT_EQ(source->GetAllocatedBlockCount(), counts.considered);
  ASSERT_TRUE(counts.candidates > 0 && counts.candidates < counts.considered);      // an eighth of the voxels
  ASSERT_EQ(counts.candidates, counts.fused);
  ASSERT_EQ(counts.candidates, counts.allocated);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.sampled > 10000);
  ASSERT_EQ(counts.candidates, coarse->GetAllocatedBlockCount());
  ASSERT_EQ(size_t(0), coarse->GetVisibleBlocks().GetSize());        // until the next SetView

  coarse->SetView(frame, 3);
  Frame traced;
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(coarse);
  tracer.Trace(traced);
  std::vector<float> depths(traced.depth_image->GetTotal());
  traced.depth_image->CopyToHost(depths.data());
  int hits = 0;
  double error = 0;
  for (int y = 0; y < kHeight; ++y)
    for (int x = 0; x < kWidth; ++x)
    {
      const float depth = depths[size_t(y) * kWidth + x];
      if (!(depth > 0)) continue;
      ++hits;
      error += std::fabs(depth - (1.5f + 0.001f * x + 0.0007f * y));
    }
  std::printf("         %d of %d pixels hit, mean |depth error| %.5f m\n", hits, kWidth * kHeight, hits ? error / hits : 0.0);
  ASSERT_TRUE(hits > kWidth * kHeight / 2);
  ASSERT_TRUE(error / hits < 0.008);
}

// equal voxel and truncation lengths, one sample point: Merge(other, Tdst_src), byte for byte
TEST(Resample, EqualLengthsGiveTheMergeThroughAPose)
{
  const Frame left = SlantedFrame(Transform());
  const Frame right = SlantedFrame(Transform::Translate(0.3f, 0.0f, 0.0f));
  auto posed = Fused(8192, 2048, left, 2);
  auto resampled = Fused(8192, 2048, left, 2);
  auto b = Fused(4093, 4096, right, 3);            // another table size
  const float yaw = 0.5f * 0.17453293f;            // 10 degrees
  const Transform pose = Transform::Translate(0.013f, -0.021f, 0.008f) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f);
  const MergePoseCounts want = posed->Merge(*b, pose);
  const MergePoseCounts got = resampled->MergeResampled(*b, pose, 1);
  ASSERT_EQ(want.considered, got.considered);
  ASSERT_EQ(want.candidates, got.candidates);
  ASSERT_EQ(want.fused, got.fused);
  ASSERT_EQ(want.allocated, got.allocated);
  ASSERT_EQ(want.left_out, got.left_out);
  ASSERT_EQ(want.rounds, got.rounds);
  ASSERT_EQ(want.sampled, got.sampled);
  ASSERT_TRUE(got.sampled > 100000);
  const std::vector<vk_hash_entry> entries_posed = Entries(*posed), entries_resampled = Entries(*resampled);
  const std::vector<vk_voxel> voxels_posed = Voxels(*posed), voxels_resampled = Voxels(*resampled);
  ASSERT_TRUE(std::memcmp(entries_posed.data(), entries_resampled.data(), sizeof(vk_hash_entry) * entries_posed.size()) == 0);
  ASSERT_TRUE(std::memcmp(voxels_posed.data(), voxels_resampled.data(), sizeof(vk_voxel) * voxels_posed.size()) == 0);
  // the default number of sample points at equal lengths is that one
  auto again = Fused(8192, 2048, left, 2);
  ASSERT_EQ(want.sampled, again->MergeResampled(*b, pose).sampled);
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in either volume;
// never into itself; voxel lengths no more than a factor of 4 apart; 0 .. 4 sample points per axis
TEST(Resample, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  auto coarse = std::make_shared<Volume>(4093, 2048);
  coarse->SetVoxelLength(2.0f * kVoxel);
  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = SlantedFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int before = volume->GetAllocatedBlockCount();
  ASSERT_THROW(coarse->MergeResampled(*volume, Transform()));
  ASSERT_THROW(volume->MergeResampled(*coarse, Transform()));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_EQ(0, coarse->GetAllocatedBlockCount());
  volume->CancelRequestsAhead(3);
  ASSERT_THROW(volume->MergeResampled(*volume, Transform()));
  ASSERT_THROW(coarse->MergeResampled(*volume, Transform(), 5));
  auto far = std::make_shared<Volume>(509, 64);
  far->SetVoxelLength(5.0f * kVoxel);
  ASSERT_THROW(far->MergeResampled(*volume, Transform()));
  ASSERT_EQ(0, coarse->GetAllocatedBlockCount());
  const MergePoseCounts counts = coarse->MergeResampled(*volume, Transform());
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.fused > 0);
}

int main(int argc, char** argv) { return RunTests("resample_tests", argc, argv); }
