// release_tests.cpp — Volume::ReleaseBlocks through the C++ class layer -> C ABI -> HIP kernels (no upstream case: the
// reference's volume only grows, src/volume.cu:304-368). The call's exact outcome is held against its CPU statement by
// tests/test_gpu_release.py; these cases are what a user of the class sees: blocks come back, an exhausted volume
// allocates again, and the call refuses to run on top of an announced frame. Harness: volume_test_support.h.
//
//   ./release_tests            run everything (needs a GPU)
//   ./release_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// a box release frees what lies outside the box, and nothing else
TEST(Release, BoxFreesWhatLiesOutside)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = std::make_shared<Volume>(8192, 2048);
  volume->SetVoxelLength(0.008f);
  for (int i = 0; i < 6; ++i) volume->SetView(frame);
  DepthIntegrator integrator(volume);
  integrator.Integrate(frame);
  const int before = volume->GetAllocatedBlockCount();
  int outside = 0;
  for (const vk_hash_entry& e : Entries(*volume)) outside += (e.data >= 0 && e.block.origin[0] < 0) ? 1 : 0;
  ASSERT_TRUE(before > 500 && outside > 100 && outside < before);

  ReleaseRule rule;
  rule.outside_box = true;                       // keep the half space x >= 0
  rule.keep_lo[0] = 0;      rule.keep_lo[1] = -32768; rule.keep_lo[2] = -32768;
  rule.keep_hi[0] = 32767;  rule.keep_hi[1] = 32767;  rule.keep_hi[2] = 32767;
  const ReleaseCounts counts = volume->ReleaseBlocks(rule);
  ASSERT_EQ(outside, counts.released);
  ASSERT_EQ(before - outside, counts.kept);
  ASSERT_EQ(8192 + 2048 - counts.kept, counts.free_slots);
  ASSERT_EQ(before - counts.released, volume->GetAllocatedBlockCount());
  int left = 0;
  for (const vk_hash_entry& e : Entries(*volume))
  {
    if (e.data < 0) continue;
    ++left;
    ASSERT_TRUE(e.block.origin[0] >= 0);
  }
  ASSERT_EQ(counts.kept, left);
  ASSERT_EQ(size_t(0), volume->GetVisibleBlocks().GetSize());      // until the next SetView
  // the volume goes on: the same view brings the released blocks back
  for (int i = 0; i < 6; ++i) volume->SetView(frame);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_TRUE(volume->GetVisibleBlocks().GetSize() > 500);
}

// Volume(509, 96) in front of a frame that asks for a thousand blocks runs dry; a release gives it room to allocate again
TEST(Release, ExhaustedVolumeAllocatesAgain)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = std::make_shared<Volume>(509, 96);
  volume->SetVoxelLength(0.008f);
  for (int i = 0; i < 8; ++i) volume->SetView(frame);
  DepthIntegrator integrator(volume);
  integrator.Integrate(frame);
  int32_t counters[VK_CTR_PUBLIC];
  volume->GetCounters(counters);                  // POOL EXHAUSTED, in fuse_sequence's words
  const int dropped = counters[VK_CTR_DROPPED];
  ASSERT_TRUE(dropped > 0 && counters[VK_CTR_VOXEL_PTR] < -1);
  ASSERT_EQ(509 + 96, volume->GetAllocatedBlockCount());

  ReleaseRule rule;
  rule.unobserved = true;
  rule.no_surface = true;
  rule.min_abs_distance = 0.75f;
  const ReleaseCounts counts = volume->ReleaseBlocks(rule);
  ASSERT_TRUE(counts.released > 0 && counts.kept > 0);
  ASSERT_EQ(509 + 96, counts.kept + counts.free_slots);            // leaked slots included
  ASSERT_TRUE(counts.excess_entries <= 96);
  ASSERT_EQ(counts.kept, volume->GetAllocatedBlockCount());
  volume->GetCounters(counters);
  ASSERT_EQ(dropped, counters[VK_CTR_DROPPED]);                    // untouched
  ASSERT_EQ(counts.free_slots - 1, counters[VK_CTR_VOXEL_PTR]);
  ASSERT_EQ(509 + counts.excess_entries, counters[VK_CTR_EXCESS_PTR]);

  // elsewhere: the camera has moved on
  const Frame next = SlantedFrame(Transform::Translate(0.0f, 0.0f, 1.0f));
  volume->SetView(next, 3);
  ASSERT_TRUE(volume->GetAllocatedBlockCount() > counts.kept);
  ASSERT_TRUE(volume->GetVisibleBlocks().GetSize() > 0);
  integrator.Integrate(next);
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in the volume
TEST(Release, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = std::make_shared<Volume>(8192, 2048);
  volume->SetVoxelLength(0.008f);
  volume->SetView(frame, 3);
  DepthIntegrator integrator(volume);
  integrator.Integrate(frame);
  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = SlantedFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int before = volume->GetAllocatedBlockCount();
  ASSERT_THROW(volume->ReleaseBlocks(ReleaseRule()));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  volume->CancelRequestsAhead(3);
  const int announced = volume->GetAllocatedBlockCount();
  const ReleaseCounts counts = volume->ReleaseBlocks(ReleaseRule());
  ASSERT_EQ(0, counts.released);
  ASSERT_EQ(announced, counts.kept);
}

int main(int argc, char** argv) { return RunTests("release_tests", argc, argv); }
