// sample_tests.cpp — Volume::Sample(points, count, samples, gradients, pose) through the C++ class layer -> C ABI -> HIP kernel
// (no upstream case: the reference samples its volume only along camera rays). The call is held against the CPU statement
// bit for bit by tests/test_gpu_sample.py; these cases are what a user of the class sees: a voxel's centre gives the stored
// voxel, the vertices the Extractor makes lie on the zero set of the sampled field, and a merge through a pose into a fresh
// volume is the samples of its voxels' centres. Harness: volume_test_support.h.
//
//   ./sample_tests            run everything (needs a GPU)
//   ./sample_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// the centres of the 512 voxels of every block of the volume, in voxels, and where each voxel is in the pool
static void Centres(const std::vector<vk_hash_entry>& entries, std::vector<Vector3f>* centres, std::vector<size_t>* at)
{
  for (const vk_hash_entry& e : entries)
  {
    if (e.data < 0) continue;
    for (int i = 0; i < VK_BLOCK_VOXELS; ++i)
    {
      centres->push_back(Vector3f(float(8 * e.block.origin[0] + (i & 7)) + 0.5f, float(8 * e.block.origin[1] + ((i >> 3) & 7)) + 0.5f,
          float(8 * e.block.origin[2] + (i >> 6)) + 0.5f));
      at->push_back(size_t(e.data) * VK_BLOCK_VOXELS + i);
    }
  }
}

// the samples (and the gradients, when asked for) at host points
static std::vector<vk_voxel> SampleAt(const Volume& volume, const std::vector<Vector3f>& points, const Transform* pose,
    const SampleOptions& options, std::vector<Vector4f>* gradients = nullptr)
{
  Buffer<Vector3f> points_dev(points.size());
  Buffer<Voxel> samples_dev(points.size());
  Buffer<Vector4f> gradients_dev(gradients ? points.size() : 0);
  points_dev.CopyFromHost(points.data());
  volume.Sample(points_dev.GetData(), int(points.size()), samples_dev.GetData(), gradients ? gradients_dev.GetData() : nullptr, pose, options);
  std::vector<vk_voxel> samples(points.size());
  samples_dev.CopyToHost(reinterpret_cast<Voxel*>(samples.data()));
  if (gradients)
  {
    gradients->resize(points.size());
    gradients_dev.CopyToHost(gradients->data());
  }
  return samples;
}

// in voxel units a centre is exact: the sample there is the voxel's own 20 bytes wherever it has a weight, and Voxel::Empty() elsewhere
TEST(Sample, VoxelCentresGiveTheStoredVoxels)
{
  auto volume = Fused(509, 4096, BumpsFrame(Transform()), 2);
  const std::vector<vk_hash_entry> entries = Entries(*volume);
  const std::vector<vk_voxel> voxels = Voxels(*volume);
  std::vector<Vector3f> centres;
  std::vector<size_t> at;
  Centres(entries, &centres, &at);
  SampleOptions options;
  options.voxel_units = true;
  std::vector<Vector4f> gradients;
  const std::vector<vk_voxel> samples = SampleAt(*volume, centres, nullptr, options, &gradients);
  const Voxel none = Voxel::Empty();
  int weighted = 0, empty = 0, with_gradient = 0;
  for (size_t i = 0; i < centres.size(); ++i)
  {
    const vk_voxel& stored = voxels[at[i]];
    if (stored.distance_weight != 0)
    {
      ++weighted;
      ASSERT_TRUE(std::memcmp(&samples[i], &stored, sizeof(vk_voxel)) == 0);
    }
    else
    {
      ++empty;
      ASSERT_TRUE(std::memcmp(&samples[i], &none, sizeof(vk_voxel)) == 0);
    }
    const float valid = gradients[i][3];
    ASSERT_TRUE(valid == 0.0f || valid == 1.0f);
    if (valid == 0.0f) ASSERT_TRUE(gradients[i][0] == 0.0f && gradients[i][1] == 0.0f && gradients[i][2] == 0.0f);
    else ++with_gradient;
  }
  std::printf("         %d weighted voxels, %d without a weight, %d gradients\n", weighted, empty, with_gradient);
  ASSERT_TRUE(weighted > 100000 && empty > 1000 && with_gradient > 50000);
  // a null output is allowed, two are not, and neither is a count below zero
  Buffer<Vector3f> points_dev(8);
  Buffer<Voxel> samples_dev(8);
  ASSERT_THROW(volume->Sample(points_dev.GetData(), 8, nullptr, nullptr));
  ASSERT_THROW(volume->Sample(points_dev.GetData(), -1, samples_dev.GetData(), nullptr));
  volume->Sample(nullptr, 0, samples_dev.GetData(), nullptr);
}

// the Extractor puts a vertex where the distance interpolated along a lattice edge is zero: on an edge the trilinear
// sample is that interpolation, so the sampled distance there is zero but for rounding (1e-4: the README's TSDF tolerance)
TEST(Sample, MeshVerticesLieOnTheZeroSet)
{
  auto volume = Fused(509, 4096, BumpsFrame(Transform()), 2);
  Extractor extractor(volume);
  extractor.SetAllAllocated(true);
  DeviceMesh mesh;
  extractor.Extract(mesh);
  const int count = int(mesh.points.GetSize());
  ASSERT_TRUE(count > 10000);
  Buffer<Voxel> samples_dev(count);
  SampleOptions options;
  options.distance_only = true;
  volume->Sample(mesh.points.GetData(), count, samples_dev.GetData(), nullptr, nullptr, options);
  std::vector<vk_voxel> samples(count);
  samples_dev.CopyToHost(reinterpret_cast<Voxel*>(samples.data()));
  float worst = 0.0f;
  for (const vk_voxel& s : samples)
  {
    ASSERT_TRUE(s.distance_weight != 0);
    ASSERT_TRUE(s.color_weight == 0 && s.color[0] == 0.0f && s.color[1] == 0.0f && s.color[2] == 0.0f);
    worst = std::fmax(worst, std::fabs(s.distance));
  }
  std::printf("         %d vertices, worst |D| %g\n", count, worst);
  ASSERT_TRUE(worst <= 1e-4f);
}

// Merge(source, pose) into a fresh volume: every voxel of every block it allocates is the sample of the source at the
// voxel's centre carried back, passed through the running average from weight 0 — the value itself, the weight capped at 16
TEST(Sample, AFreshMergeIsTheSamplesOfItsCentres)
{
  auto source = Fused(509, 4096, BumpsFrame(Transform()), 3);
  const float yaw = 0.5f * 0.17453293f, pitch = 0.5f * 0.08726646f;   // 10 and 5 degrees
  const Transform pose = Transform::Translate(0.013f, -0.021f, 0.008f) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f) *
      Transform::Rotate(std::cos(pitch), std::sin(pitch), 0.0f, 0.0f);
  auto fresh = Fresh(4093, 4096);
  const MergePoseCounts counts = fresh->Merge(*source, pose);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.sampled > 100000);
  const std::vector<vk_hash_entry> entries = Entries(*fresh);
  const std::vector<vk_voxel> voxels = Voxels(*fresh);
  std::vector<Vector3f> centres;
  std::vector<size_t> at;
  Centres(entries, &centres, &at);
  ASSERT_EQ(size_t(counts.fused) * VK_BLOCK_VOXELS, centres.size());
  SampleOptions options;
  options.voxel_units = true;
  const Transform back = pose.Inverse();
  const std::vector<vk_voxel> samples = SampleAt(*source, centres, &back, options);
  int sampled = 0;
  for (size_t i = 0; i < centres.size(); ++i)
  {
    vk_voxel want = samples[i];
    if (want.distance_weight > 16) want.distance_weight = 16;
    if (want.color_weight > 16) want.color_weight = 16;
    if (want.distance_weight != 0) ++sampled;
    ASSERT_TRUE(std::memcmp(&want, &voxels[at[i]], sizeof(vk_voxel)) == 0);
  }
  std::printf("         %d blocks, %d voxels took a distance sample\n", counts.fused, sampled);
  ASSERT_EQ(counts.sampled, sampled);
}

int main(int argc, char** argv) { return RunTests("sample_tests", argc, argv); }
