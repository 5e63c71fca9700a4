// tsdf_volume.cpp — Volume host class over vk_volume_* (ref: src/volume.cu:370-627).
#include <vulcan/tsdf_volume.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <vulcan/block.h>
#include <vulcan/exception.h>
#include <vulcan/observation.h>
#include <vulcan/hash.h>
#include <vulcan/voxel.h>

namespace vulcan
{

Volume::Volume(int main_block_count, int excess_block_count) :
  depth_range_(0.1f, 5.0f),
  max_block_count_(main_block_count + excess_block_count),
  main_block_count_(main_block_count),
  excess_block_count_(excess_block_count),
  truncation_length_(0.04f),
  voxel_length_(0.008f),
  empty_(true),
  visible_count_stale_(false),
  request_stream_(nullptr),
  requested_(nullptr),
  integrated_(nullptr),
  integrated_recorded_(false),
  normals_late_(nullptr)
{
  std::memset(&view_bounds_, 0, sizeof(view_bounds_));
  std::memset(&light_prep_, 0, sizeof(light_prep_));
  std::memset(&requests_ahead_, 0, sizeof(requests_ahead_));
  Initialize();
}

Volume::~Volume()
{
#ifndef NDEBUG
  // a pool that ran dry is said once before the volume goes (debug builds; a blocking readback is harmless here)
  if (!empty_ && !pool_exhaustion_noted_ && counters_.GetData())
  {
    int32_t counters[VK_CTR_PUBLIC];
    const vk_volume v = ToVk();
    if (vk_volume_read_counters_sync(&v, counters, Device::GetStream()) == VK_OK) NotePoolExhaustion(counters[VK_CTR_DROPPED]);
  }
#endif
  if (normals_late_) (void)vk_free_host(normals_late_);
  if (request_stream_)
  {
    (void)vk_stream_synchronize(request_stream_);
    (void)vk_event_destroy(requested_);
    (void)vk_event_destroy(integrated_);
    (void)vk_stream_destroy(request_stream_);
  }
}

int Volume::GetMainBlockCount() const { return main_block_count_; }

int Volume::GetExcessBlockCount() const { return excess_block_count_; }

const Vector2f& Volume::GetDepthRange() const { return depth_range_; }

void Volume::SetDepthRange(const Vector2f& range)
{
  VULCAN_DEBUG(range[0] > 0 && range[0] < range[1]);
  depth_range_ = range;
}

void Volume::SetDepthRange(float min, float max) { SetDepthRange(Vector2f(min, max)); }

float Volume::GetVoxelLength() const { return voxel_length_; }

void Volume::SetVoxelLength(float length)
{
  VULCAN_DEBUG(length > 0);
  voxel_length_ = length;
}

float Volume::GetTruncationLength() const { return truncation_length_; }

void Volume::SetTruncationLength(float length)
{
  VULCAN_DEBUG(length > 0);
  truncation_length_ = length;
}

vk_volume Volume::ToVk() const
{
  vk_volume v;
  v.voxels = reinterpret_cast<vk_voxel*>(const_cast<Voxel*>(voxels_.GetData()));
  v.hash_entries = reinterpret_cast<vk_hash_entry*>(const_cast<HashEntry*>(hash_entries_.GetData()));
  v.free_voxel_blocks = const_cast<int*>(free_voxel_blocks_.GetData());
  v.allocation_types = reinterpret_cast<uint8_t*>(const_cast<AllocationType*>(allocation_types_.GetData()));
  v.allocation_blocks = reinterpret_cast<vk_block*>(const_cast<Block*>(allocation_blocks_.GetData()));
  v.block_visibility = reinterpret_cast<uint8_t*>(const_cast<Visibility*>(block_visibility_.GetData()));
  v.visible_blocks = const_cast<int*>(visible_blocks_.GetData());
  v.counters = const_cast<int*>(counters_.GetData());
  v.main_block_count = main_block_count_;
  v.excess_block_count = excess_block_count_;
  v.voxel_length = voxel_length_;
  v.truncation_length = truncation_length_;
  v.min_depth = depth_range_[0];
  v.max_depth = depth_range_[1];
  return v;
}

vk_view_bounds* Volume::GetViewBounds() const { return view_bounds_.scratch ? &view_bounds_ : nullptr; }

void Volume::AttachViewBounds(float* scratch, int bounds_width, int bounds_height, const Vector2f& depth_range) const
{
  std::memset(&view_bounds_, 0, sizeof(view_bounds_));
  // the pinned word a normals workgroup of Tracer::Trace(keyframe, next_frame) sets when its bounded wait expires
  // (vk.h vk_view_bounds.late_host): the next Trace, or Tracer::SettleNormals, then throws instead of leaving wrong normals
  if (!normals_late_)
  {
    void* word = nullptr;
    VK_ASSERT(vk_malloc_host(&word, sizeof(int32_t)));
    normals_late_ = static_cast<int32_t*>(word);
  }
  *normals_late_ = 0;
  view_bounds_.late_host = normals_late_;
  view_bounds_.scratch = scratch;
  view_bounds_.bounds_width = bounds_width;
  view_bounds_.bounds_height = bounds_height;
  view_bounds_.min_depth = depth_range[0];
  view_bounds_.max_depth = depth_range[1];
}

void Volume::DetachViewBounds(const float* scratch) const
{
  if (view_bounds_.scratch == scratch) std::memset(&view_bounds_, 0, sizeof(view_bounds_));
}

void Volume::CancelRequestsAhead(int rounds)
{
  if (requests_ahead_.valid != 1) return;
  view_bounds_.valid = 0;
  const vk_volume v = ToVk();
  VK_ASSERT(vk_requests_ahead_cancel(&v, &requests_ahead_, rounds, Device::GetStream()));
  visible_count_stale_ = true;
  empty_ = false;
}

vk_light_prep* Volume::GetLightPreparation() const { return light_prep_.mask ? &light_prep_ : nullptr; }

void Volume::AttachLightPreparation(float* mask, float* records, int capacity_pixels, float depth_threshold) const
{
  std::memset(&light_prep_, 0, sizeof(light_prep_));
  light_prep_.mask = mask;
  light_prep_.records = records;
  light_prep_.capacity = capacity_pixels;
  light_prep_.depth_threshold = depth_threshold;
}

void Volume::DetachLightPreparation(const float* mask) const
{
  if (light_prep_.mask == mask) std::memset(&light_prep_, 0, sizeof(light_prep_));
}

void Volume::SetView(const Frame& frame) { SetView(frame, 1); }

void Volume::SetView(const Frame& frame, int rounds)
{
  view_bounds_.valid = 0;   // the visible list is about to change
  VULCAN_ASSERT_MSG(frame.depth_image, "missing depth image");
  VULCAN_ASSERT_MSG(rounds >= 1, "SetView needs at least one round");
  const vk_volume v = ToVk();
  const vk_frame f = frame.ToVk();
  if (request_stream_)
  {
    VULCAN_ASSERT_MSG(requests_ahead_.valid != 1, "a request pass made ahead and a request stream exclude each other");
    if (integrated_recorded_) VK_ASSERT(vk_stream_wait_event(request_stream_, integrated_));
    VK_ASSERT(vk_volume_set_view_rounds_split(&v, &f, GetLightPreparation(), rounds, request_stream_, requested_, Device::GetStream()));
  }
  else
  {
    // (with a record that is not valid this is vk_volume_set_view_rounds)
    const int code = vk_volume_set_view_rounds_ahead(&v, &f, GetLightPreparation(), rounds, &requests_ahead_, Device::GetStream());
    VULCAN_ASSERT_MSG(!(code == VK_ERR_ARGUMENT && requests_ahead_.valid == 1),
        "SetView of another frame than the one Tracer::Trace(keyframe, next_frame) announced");
    VK_ASSERT(code);
  }
  visible_count_stale_ = true;
  empty_ = false;
}

bool Volume::SetViewAtDevicePose(const Frame& frame, const vk_transform* pose_device, int rounds)
{
  VULCAN_ASSERT_MSG(frame.depth_image, "missing depth image");
  VULCAN_ASSERT_MSG(rounds >= 1 && pose_device, "SetViewAtDevicePose needs a device pose and at least one round");
  if (request_stream_ || requests_ahead_.valid == 1) return false;
  const vk_volume v = ToVk();
  const vk_frame f = frame.ToVk();
  vk_light_prep* prep = GetLightPreparation();
  if (prep && prep->normals_out) return false;
  const int code = vk_volume_set_view_at_device_pose(&v, &f, pose_device, prep, rounds, Device::GetStream());
  if (code == VK_ERR_UNSUPPORTED) return false;
  VK_ASSERT(code);
  view_bounds_.valid = 0;   // the visible list has changed
  visible_count_stale_ = true;
  empty_ = false;
  return true;
}

void Volume::EnableRequestStream()
{
  if (request_stream_) return;
  VK_ASSERT(vk_stream_create(&request_stream_));
  VK_ASSERT(vk_event_create_ordering(&requested_, 1));    // behind a pass that WRITES what the waiting stream reads (vk.h)
  VK_ASSERT(vk_event_create_ordering(&integrated_, 0));
  integrated_recorded_ = false;
}

void Volume::NoteIntegrated() const
{
  if (!request_stream_) return;
  VK_ASSERT(vk_event_record(integrated_, Device::GetStream()));
  integrated_recorded_ = true;
}

void Volume::ComputeNormalsAndSetView(Frame& frame, int rounds)
{
  if (requests_ahead_.valid == 1 && requests_ahead_.normals_made == 1)
  {
    // Tracer::Trace(keyframe, frame, true) announced this frame and its normals came with the pass: nothing is due.
    // (Stamping the normal image again would give the frame a content id the record does not name; another frame
    // than the announced one is refused by SetView.)
    SetView(frame, rounds);
    return;
  }
  if (requests_ahead_.valid == 1)
  {
    // Announced WITHOUT its normals (Tracer::Trace(keyframe, frame) — next_needs_normals defaults to false): they are
    // still due (this used to be skipped on the record's validity alone, and LightIntegrator then shaded from
    // a stale or uninitialised normal image, silently). The record names the frame by its images' stamps, so the normal
    // image is written in place without a new stamp (a kernel launch, as Frame::ComputeNormals; ref: src/frame.cpp:21-36),
    // the announced SetView runs, and whatever the pass prepared from the OLD normals is void: LightIntegrator::Integrate
    // then prepares again (vk_light_prepare) from the new ones.
    VULCAN_ASSERT_MSG(frame.depth_image, "missing depth image");
    const int w = frame.depth_image->GetWidth(), h = frame.depth_image->GetHeight();
    const bool sized = frame.normal_image && frame.normal_image->GetWidth() == w && frame.normal_image->GetHeight() == h;
    // (a frame announced without a normal image of its size cannot have had a preparation riding: prep_rides needs one,
    // and a new image is new content — SetView below then refuses the frame, as for any frame that was not announced)
    if (!sized) { frame.ComputeNormals(); SetView(frame, rounds); return; }
    const ColorImage& normals = *frame.normal_image;                  // const view: no new stamp
    const vk_projection k = frame.depth_projection.ToVk();
    const Image& depths = *frame.depth_image;
    VK_ASSERT(vk_frame_compute_normals(depths.GetData(), &k,
        const_cast<float*>(reinterpret_cast<const float*>(normals.GetData())), w, h, Device::GetStream()));
    vk_light_prep* made = GetLightPreparation();
    SetView(frame, rounds);
    if (made) made->valid = 0;
    return;
  }
  vk_light_prep* prep = GetLightPreparation();
  if (!prep)
  {
    frame.ComputeNormals();
    SetView(frame, rounds);
    return;
  }
  VULCAN_ASSERT_MSG(frame.depth_image, "missing depth image");
  if (!frame.normal_image) frame.normal_image = std::make_shared<ColorImage>();
  frame.normal_image->Resize(frame.depth_image->GetWidth(), frame.depth_image->GetHeight());
  prep->normals_out = reinterpret_cast<float*>(frame.normal_image->GetData());   // (GetData stamps the image: new content)
  SetView(frame, rounds);
}

const Buffer<HashEntry>& Volume::GetHashEntries() const { return hash_entries_; }

const Buffer<int>& Volume::GetAllocatedBlocks() const
{
  VULCAN_THROW("not implemented");  // as in the reference (volume.cu:444-448)
}

const Buffer<int>& Volume::GetVisibleBlocks() const
{
  if (visible_count_stale_)
  {
    visible_blocks_.Resize(GetBufferSize());  // volume.cu:494, deferred to first use
    visible_count_stale_ = false;
  }
  return visible_blocks_;
}

const Buffer<Voxel>& Volume::GetVoxels() const { return voxels_; }

Buffer<Voxel>& Volume::GetVoxels() { return voxels_; }

void Volume::GetCounters(int32_t* counters) const
{
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_read_counters_sync(&v, counters, Device::GetStream()));
  NotePoolExhaustion(counters[VK_CTR_DROPPED]);
}

// Upstream asserts on the device, in debug builds, when the pool runs dry (VULCAN_DEBUG_MSG "voxel memory exhausted" /
// "excess memory exhausted", src/volume.cu:338,353) and drops the request silently otherwise. Here the dropped requests are
// counted on the device (VK_CTR_DROPPED) and never leave it inside the frame loop, so the note is made where the class
// already reads the counters: once per volume, on stderr, in builds without NDEBUG — upstream's condition for its message.
void Volume::NotePoolExhaustion(int32_t dropped) const
{
#ifndef NDEBUG
  if (dropped > 0 && !pool_exhaustion_noted_)
  {
    pool_exhaustion_noted_ = true;
    std::fprintf(stderr, "vulcan::Volume: voxel / excess memory exhausted: %d allocation requests dropped so far "
        "(pool of %d + %d blocks; ref: src/volume.cu:338,353)\n", dropped, main_block_count_, excess_block_count_);
  }
#else
  (void)dropped;
#endif
}

int Volume::GetAllocatedBlockCount() const
{
  int32_t counters[VK_CTR_PUBLIC];
  GetCounters(counters);
  // the free-slot pointer keeps falling below -1 once the pool is empty, as upstream's does (src/volume.cu:352-356)
  const int taken = max_block_count_ - 1 - counters[VK_CTR_VOXEL_PTR];
  return taken < max_block_count_ ? taken : max_block_count_;
}

void Volume::AssertNoFrameAnnounced() const
{
  VULCAN_ASSERT_MSG(requests_ahead_.valid != 1, "a frame announced by Tracer::Trace(keyframe, next_frame) has its requests in the volume: SetView(that frame) or CancelRequestsAhead() first");
}

const vk_transform* Volume::PoseOnDevice(const Transform* pose) const
{
  if (!pose) return nullptr;
  if (sample_pose_.GetSize() == 0) sample_pose_.Resize(32);
  const vk_transform seed = pose->ToVk();
  vk_transform* pose_dev = reinterpret_cast<vk_transform*>(sample_pose_.GetData());
  VK_ASSERT(vk_transform_upload(pose_dev, &seed, Device::GetStream()));
  return pose_dev;
}

void Volume::VoidMadeAhead() const
{
  view_bounds_.valid = 0;
  light_prep_.valid = 0;
}

void Volume::EmptyVisibleList() const
{
  visible_blocks_.Resize(0);
  visible_count_stale_ = false;
}

int Volume::RayFlags(bool voxel_units, bool one_observation)
{
  return (voxel_units ? VK_RAYS_VOXEL_UNITS : 0) | (one_observation ? VK_RAYS_ONE_OBSERVATION : 0);
}

void Volume::Sized(Buffer<unsigned char>& workspace, size_t bytes, Buffer<int>& counts, size_t count)
{
  if (bytes != 0 && workspace.GetSize() != bytes) workspace.Resize(bytes);
  if (counts.GetSize() == 0) counts.Resize(count);
}

std::array<int32_t, 8> Volume::EightCounts(const Buffer<int>& counts_dev)
{
  std::array<int32_t, 8> counts;
  counts_dev.CopyToHost(counts.data());
  return counts;
}

void Volume::RegistrationBuffers::Begin(const Transform* seed)
{
  static_assert(sizeof(vk_transform) == 32 * sizeof(float), "vk_transform layout");
  if (floats.GetSize() == 0) floats.Resize(32 + 48 + 8);
  if (ints.GetSize() == 0) ints.Resize(2 + 4);
  pose = reinterpret_cast<vk_transform*>(floats.GetData());
  system = floats.GetData() + 32;
  update = system + 48;
  state = ints.GetData();
  counts = state + 2;
  if (!seed) return;
  const vk_transform start = seed->ToVk();
  VK_ASSERT(vk_transform_upload(pose, &start, Device::GetStream()));
  VK_ASSERT(vk_memset(state, 0, 2 * sizeof(int), Device::GetStream()));
}

Registration Volume::RegistrationBuffers::Read() const
{
  std::vector<float> host_floats(floats.GetSize());
  std::vector<int> host_ints(ints.GetSize());
  floats.CopyToHost(host_floats.data());
  ints.CopyToHost(host_ints.data());
  vk_transform result;
  std::memcpy(&result, host_floats.data(), sizeof(result));
  Registration out;
  out.pose = Transform::FromVk(result);
  out.steps = host_ints[0];
  out.converged = host_ints[1] == 1;
  out.overlap = host_ints[1] != VK_REGISTER_NO_OVERLAP;
  out.residuals = host_ints[4];
  out.rms = host_ints[4] > 0 ? std::sqrt(host_floats[32 + 42] / float(host_ints[4])) : 0.0f;
  return out;
}

ReleaseCounts Volume::ReleaseBlocks(const ReleaseRule& rule)
{
  AssertNoFrameAnnounced();
  vk_release_rule r;
  std::memset(&r, 0, sizeof(r));
  r.flags = (rule.unobserved ? VK_RELEASE_UNOBSERVED : 0) | (rule.no_surface ? VK_RELEASE_NO_SURFACE : 0) |
            (rule.outside_box ? VK_RELEASE_OUTSIDE_BOX : 0);
  r.min_abs_distance = rule.min_abs_distance;
  for (int a = 0; a < 3; ++a)
  {
    r.keep_lo[a] = rule.keep_lo[a];
    r.keep_hi[a] = rule.keep_hi[a];
  }
  if (release_counts_.GetSize() == 0)
  {
    release_workspace_.Resize(vk_volume_release_workspace_bytes(main_block_count_, excess_block_count_));
    release_counts_.Resize(4);
  }
  VoidMadeAhead();
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_release_blocks(&v, &r, release_counts_.GetData(), release_workspace_.GetData(), Device::GetStream()));
  EmptyVisibleList();
  int32_t counts[4];
  release_counts_.CopyToHost(counts);
  ReleaseCounts out;
  out.released = counts[0];
  out.kept = counts[1];
  out.excess_entries = counts[2];
  out.free_slots = counts[3];
  return out;
}

static vk_merge_params ToVkMergeParams(const MergeOptions& options)
{
  vk_merge_params p;
  p.flags = options.skip_unobserved ? VK_MERGE_SKIP_UNOBSERVED : 0;
  p.max_rounds = options.max_rounds;
  p.max_distance_weight = options.max_distance_weight;
  p.max_color_weight = options.max_color_weight;
  return p;
}

template <typename Call>
void Volume::MergeRounds(const Volume* other, vk_merge_params& merge, Buffer<unsigned char>& workspace, size_t bytes,
    Buffer<int>& counts_dev, int count, int32_t* total, Call call)
{
  AssertNoFrameAnnounced();
  if (other) other->AssertNoFrameAnnounced();
  VULCAN_ASSERT_MSG(other != this, "a volume cannot be merged into itself");
  Sized(workspace, bytes, counts_dev, size_t(count));
  VoidMadeAhead();
  const vk_volume dst = ToVk(), source = other ? other->ToVk() : dst;
  const vk_volume* src = other ? &source : nullptr;
  int32_t counters[VK_CTR_PUBLIC];
  GetCounters(counters);
  const int32_t dropped = counters[VK_CTR_DROPPED];
  // the counts: considered, [candidates,] fused, allocated, left out, rounds that posted, skipped[, sampled]
  const int k = count == 8 ? 1 : 0, fused = 1 + k, allocated = 2 + k, left_out = 3 + k, rounds = 4 + k;
  for (bool first = true;; first = false)
  {
    VK_ASSERT(call(&dst, src, counts_dev.GetData(), workspace.GetData()));
    int32_t counts[8];
    counts_dev.CopyToHost(counts);
    if (first)
      std::memcpy(total, counts, size_t(count) * sizeof(int32_t));     // considered, candidates and skipped are the first call's
    else
    {
      total[fused] += counts[fused];
      total[allocated] += counts[allocated];
      total[left_out] = counts[left_out];
      total[rounds] += counts[rounds];
      if (count == 8) total[7] += counts[7];
    }
    // every block (candidate) once: while a call posted in all its rounds, dropped nothing and still left some out, the
    // next call goes on with those
    GetCounters(counters);
    if (!(counts[rounds] == merge.max_rounds && counts[left_out] > 0 && counters[VK_CTR_DROPPED] == dropped)) break;
    merge.flags |= VK_MERGE_CONTINUE;
  }
  NotePoolExhaustion(counters[VK_CTR_DROPPED]);
  EmptyVisibleList();
}

MergeCounts Volume::Merge(const Volume& other, const MergeOptions& options)
{
  vk_merge_params p = ToVkMergeParams(options);
  int32_t counts[6];
  MergeRounds(&other, p, merge_workspace_, vk_volume_merge_workspace_bytes(other.main_block_count_, other.excess_block_count_),
      merge_counts_, 6, counts, [&p](const vk_volume* dst, const vk_volume* src, int32_t* counts_dev, void* workspace)
      { return vk_volume_merge(dst, src, &p, counts_dev, workspace, Device::GetStream()); });
  MergeCounts out;
  out.considered = counts[0];
  out.fused = counts[1];
  out.allocated = counts[2];
  out.left_out = counts[3];
  out.rounds = counts[4];
  out.skipped = counts[5];
  return out;
}

MergePoseCounts Volume::Merge(const Volume& other, const Transform& Tdst_src, const MergeOptions& options)
{
  vk_merge_pose_params p;
  p.merge = ToVkMergeParams(options);
  p.pose = Tdst_src.ToVk();                       // the matrix and its inverse, from the one Transform
  int32_t counts[8];
  MergeRounds(&other, p.merge, merge_pose_workspace_, vk_volume_merge_posed_workspace_bytes(other.main_block_count_,
      other.excess_block_count_, main_block_count_, excess_block_count_), merge_pose_counts_, 8, counts,
      [&p](const vk_volume* dst, const vk_volume* src, int32_t* counts_dev, void* workspace)
      { return vk_volume_merge_posed(dst, src, &p, counts_dev, workspace, Device::GetStream()); });
  MergePoseCounts out;
  out.considered = counts[0];
  out.candidates = counts[1];
  out.fused = counts[2];
  out.allocated = counts[3];
  out.left_out = counts[4];
  out.rounds = counts[5];
  out.skipped = counts[6];
  out.sampled = counts[7];
  return out;
}

MergePoseCounts Volume::MergeResampled(const Volume& other, const Transform& Tdst_src, int supersample, const MergeOptions& options)
{
  // the two ratios as the library takes them: one division each
  const float r_fwd = other.voxel_length_ / voxel_length_, r_back = voxel_length_ / other.voxel_length_;
  VULCAN_ASSERT_MSG(r_fwd >= 0.25f && r_fwd <= 4.0f && r_back >= 0.25f && r_back <= 4.0f,
      "the voxel lengths are more than a factor of 4 apart: chain two calls");
  VULCAN_ASSERT_MSG(supersample >= 0 && supersample <= 4, "1 .. 4 sample points per axis, or 0 for the ratio's");
  if (supersample == 0) supersample = std::min(4, std::max(1, int(std::ceil(double(r_back) - 1e-6))));
  const int box = std::min(8, int(r_fwd * 1.7320508f) + 2);           // K of vk.h: sizes the workspace
  vk_merge_resample_params p;
  p.merge = ToVkMergeParams(options);
  p.pose = Tdst_src.ToVk();                       // the matrix and its inverse, from the one Transform
  p.supersample = supersample;
  p.reserved = 0;
  int32_t counts[8];
  MergeRounds(&other, p.merge, merge_resample_workspace_, vk_volume_merge_resampled_workspace_bytes(other.main_block_count_,
      other.excess_block_count_, main_block_count_, excess_block_count_, box), merge_resample_counts_, 8, counts,
      [&p](const vk_volume* dst, const vk_volume* src, int32_t* counts_dev, void* workspace)
      { return vk_volume_merge_resampled(dst, src, &p, counts_dev, workspace, Device::GetStream()); });
  MergePoseCounts out;
  out.considered = counts[0];
  out.candidates = counts[1];
  out.fused = counts[2];
  out.allocated = counts[3];
  out.left_out = counts[4];
  out.rounds = counts[5];
  out.skipped = counts[6];
  out.sampled = counts[7];
  return out;
}

// ---- PackedVolume: a volume's blocks, compact (vk_block_pack) ----

static const char kMapMagic[8] = {'V', 'U', 'L', 'C', 'A', 'N', 'M', 'P'};
static const int32_t kMapVersion = 1;
static const size_t kMapHeaderBytes = 32, kMapBlockBytes = sizeof(vk_voxel) * VK_BLOCK_VOXELS;

PackedVolume::PackedVolume() : PackedVolume(0, 0.008f, 0.04f) {}

PackedVolume::PackedVolume(int count, float voxel_length, float truncation_length) :
  origins_(std::make_shared<Buffer<int16_t>>(size_t(count) * 4)),
  voxels_(std::make_shared<Buffer<unsigned char>>(size_t(count) * kMapBlockBytes)),
  count_(count),
  voxel_length_(voxel_length),
  truncation_length_(truncation_length)
{
}

vk_block_pack PackedVolume::ToVk() const
{
  vk_block_pack pack;
  pack.capacity = count_;
  pack.pad = 0;
  pack.origins = const_cast<int16_t*>(origins_->GetData());
  pack.voxels = reinterpret_cast<vk_voxel*>(const_cast<unsigned char*>(voxels_->GetData()));
  return pack;
}

void PackedVolume::Save(const std::string& path) const
{
  static_assert(sizeof(float) == 4 && sizeof(int32_t) == 4, "the map file's fields");
  std::vector<int16_t> origins(size_t(count_) * 4);
  std::vector<unsigned char> voxels(size_t(count_) * kMapBlockBytes);
  if (count_ > 0)
  {
    origins_->CopyToHost(origins.data());
    voxels_->CopyToHost(voxels.data());
    Device::Synchronize();
  }
  unsigned char header[kMapHeaderBytes] = {0};                 // (the file is little-endian, as every host this builds for)
  std::memcpy(header, kMapMagic, 8);
  std::memcpy(header + 8, &kMapVersion, 4);
  const int32_t count = count_;
  std::memcpy(header + 12, &count, 4);
  std::memcpy(header + 16, &voxel_length_, 4);
  std::memcpy(header + 20, &truncation_length_, 4);
  std::FILE* file = std::fopen(path.c_str(), "wb");
  VULCAN_ASSERT_MSG(file != nullptr, "cannot write the map file " + path);
  bool good = std::fwrite(header, 1, kMapHeaderBytes, file) == kMapHeaderBytes;
  good = good && std::fwrite(origins.data(), sizeof(int16_t), origins.size(), file) == origins.size();
  good = good && std::fwrite(voxels.data(), 1, voxels.size(), file) == voxels.size();
  good = (std::fclose(file) == 0) && good;
  VULCAN_ASSERT_MSG(good, "the map file " + path + " could not be written in full");
}

PackedVolume PackedVolume::Load(const std::string& path)
{
  std::FILE* file = std::fopen(path.c_str(), "rb");
  VULCAN_ASSERT_MSG(file != nullptr, "cannot read the map file " + path);
  std::vector<unsigned char> data;
  unsigned char chunk[1 << 16];
  for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), file)) > 0;) data.insert(data.end(), chunk, chunk + got);
  std::fclose(file);
  VULCAN_ASSERT_MSG(data.size() >= kMapHeaderBytes && std::memcmp(data.data(), kMapMagic, 8) == 0, path + " is not a map file (magic)");
  int32_t version, count;
  float voxel_length, truncation_length;
  std::memcpy(&version, data.data() + 8, 4);
  std::memcpy(&count, data.data() + 12, 4);
  std::memcpy(&voxel_length, data.data() + 16, 4);
  std::memcpy(&truncation_length, data.data() + 20, 4);
  VULCAN_ASSERT_MSG(version == kMapVersion, path + ": a map file of another version");
  VULCAN_ASSERT_MSG(count >= 0, path + ": a negative block count");
  VULCAN_ASSERT_MSG(data.size() == kMapHeaderBytes + size_t(count) * (8 + kMapBlockBytes), path + ": the file's length does not match its block count");
  std::vector<int16_t> origins(size_t(count) * 4);
  if (count > 0) std::memcpy(origins.data(), data.data() + kMapHeaderBytes, origins.size() * sizeof(int16_t));
  std::vector<std::array<int16_t, 3>> seen(static_cast<size_t>(count));
  for (int k = 0; k < count; ++k)
  {
    VULCAN_ASSERT_MSG(origins[size_t(k) * 4 + 3] == 0, path + ": an origin's fourth component is not 0");
    seen[size_t(k)] = {{origins[size_t(k) * 4], origins[size_t(k) * 4 + 1], origins[size_t(k) * 4 + 2]}};
  }
  std::sort(seen.begin(), seen.end());
  VULCAN_ASSERT_MSG(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), path + ": two blocks have the same origin");
  PackedVolume pack(count, voxel_length, truncation_length);
  if (count > 0)
  {
    pack.origins_->CopyFromHost(origins.data());
    pack.voxels_->CopyFromHost(data.data() + kMapHeaderBytes + size_t(count) * 8);
    Device::Synchronize();                                     // the host vectors go away
  }
  return pack;
}

PackedVolume Volume::Pack(const PackOptions& options) const
{
  vk_pack_rule rule;
  std::memset(&rule, 0, sizeof(rule));
  rule.flags = (options.skip_unobserved ? VK_PACK_SKIP_UNOBSERVED : 0) | (options.box ? VK_PACK_BOX : 0);
  for (int a = 0; a < 3; ++a)
  {
    rule.lo[a] = options.lo[a];
    rule.hi[a] = options.hi[a];
  }
  if (pack_counts_.GetSize() == 0)
  {
    pack_workspace_.Resize(vk_volume_pack_workspace_bytes(main_block_count_, excess_block_count_));
    pack_counts_.Resize(4);
  }
  const vk_volume v = ToVk();
  vk_block_pack none;
  std::memset(&none, 0, sizeof(none));                          // voxels null: the call only counts
  VK_ASSERT(vk_volume_pack(&v, &rule, &none, pack_counts_.GetData(), pack_workspace_.GetData(), Device::GetStream()));
  int32_t counts[4];
  pack_counts_.CopyToHost(counts);
  PackedVolume pack(counts[1], voxel_length_, truncation_length_);
  if (counts[1] == 0) return pack;
  const vk_block_pack into = pack.ToVk();
  VK_ASSERT(vk_volume_pack(&v, &rule, &into, pack_counts_.GetData(), pack_workspace_.GetData(), Device::GetStream()));
  pack_counts_.CopyToHost(counts);
  VULCAN_ASSERT_MSG(counts[2] == pack.Count(), "the volume changed between the call that counted its blocks and the call that packed them");
  return pack;
}

MergeCounts Volume::Merge(const PackedVolume& pack, const MergeOptions& options)
{
  AssertNoFrameAnnounced();
  const float voxel_length = pack.VoxelLength(), truncation_length = pack.TruncationLength();
  VULCAN_ASSERT_MSG(std::memcmp(&voxel_length, &voxel_length_, sizeof(float)) == 0 &&
      std::memcmp(&truncation_length, &truncation_length_, sizeof(float)) == 0,
      "the pack's voxel or truncation length is not the volume's");
  MergeCounts out = {0, 0, 0, 0, 0, 0};
  if (pack.Count() == 0) return out;                            // no blocks: no call
  vk_merge_params p = ToVkMergeParams(options);
  const vk_block_pack from = pack.ToVk();
  int32_t counts[6];
  MergeRounds(nullptr, p, merge_packed_workspace_, vk_volume_merge_packed_workspace_bytes(pack.Count()), merge_packed_counts_, 6, counts,
      [&](const vk_volume* dst, const vk_volume*, int32_t* counts_dev, void* workspace)
      { return vk_volume_merge_packed(dst, &from, pack.Count(), voxel_length, truncation_length, &p, counts_dev, workspace, Device::GetStream()); });
  out.considered = counts[0];
  out.fused = counts[1];
  out.allocated = counts[2];
  out.left_out = counts[3];
  out.rounds = counts[4];
  out.skipped = counts[5];
  return out;
}

std::shared_ptr<Volume> Volume::Load(const std::string& path, int main_block_count, int excess_block_count)
{
  const PackedVolume pack = PackedVolume::Load(path);
  auto volume = std::make_shared<Volume>(main_block_count, excess_block_count);
  volume->SetVoxelLength(pack.VoxelLength());
  volume->SetTruncationLength(pack.TruncationLength());
  MergeOptions options;
  options.max_distance_weight = options.max_color_weight = 32767.0f;
  const MergeCounts counts = volume->Merge(pack, options);
  VULCAN_ASSERT_MSG(counts.left_out == 0, "the map's blocks do not fit the volume's table sizes");
  return volume;
}

Registration Volume::Register(const Volume& other, const Transform& start, int iterations, float max_abs_distance)
{
  vk_register_params p;
  p.flags = 0;
  p.iterations = iterations;
  p.max_abs_distance = max_abs_distance;
  p.pad = 0;
  const size_t bytes = vk_volume_register_workspace_bytes(other.main_block_count_, other.excess_block_count_);
  if (register_workspace_.GetSize() != bytes) register_workspace_.Resize(bytes);
  RegistrationBuffers& b = register_;
  b.Begin(&start);
  const vk_volume dst = ToVk(), src = other.ToVk();
  VK_ASSERT(vk_volume_register(&dst, &src, b.pose, &p, b.system, b.state, b.counts, b.update, register_workspace_.GetData(),
      Device::GetStream()));
  return b.Read();
}

// the candidates on the device, and the scores and the workspace sized for them: how many poses there are
int Volume::ScorePosesBuffers(int count, const std::vector<Transform>& poses) const
{
  const int pose_count = int(poses.size());
  const size_t bytes = vk_volume_score_poses_workspace_bytes(count, pose_count);
  if (bytes != 0 && score_poses_workspace_.GetSize() != bytes) score_poses_workspace_.Resize(bytes);
  if (pose_count > 0 && score_poses_scores_.GetSize() != poses.size() * sizeof(vk_pose_score))
  {
    score_poses_scores_.Resize(poses.size() * sizeof(vk_pose_score));
    score_poses_poses_.Resize(poses.size() * 32);
  }
  if (count > 0 && pose_count > 0)                 // no rays: no upload
  {
    std::vector<vk_transform> host(poses.size());
    for (size_t k = 0; k < poses.size(); ++k) host[k] = poses[k].ToVk();
    score_poses_poses_.CopyFromHost(reinterpret_cast<const float*>(host.data()));
  }
  return pose_count;
}

std::vector<PoseScore> Volume::ScorePoses(const Ray* rays_dev, const float* ranges_dev, int count, const std::vector<Transform>& poses,
    const ScorePosesOptions& options) const
{
  static_assert(sizeof(Ray) == 6 * sizeof(float), "Ray layout");
  // the volume is only read: allowed while a frame is announced, like Sample and RegisterRays
  vk_score_poses_params p;
  p.flags = RayFlags(options.voxel_units);
  p.min_residuals = 1;
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.max_abs_distance = options.max_abs_distance;
  p.pad = 0;
  const int pose_count = ScorePosesBuffers(count, poses);
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_score_poses(&v, reinterpret_cast<const float*>(rays_dev), ranges_dev, count,
      reinterpret_cast<const vk_transform*>(score_poses_poses_.GetData()), pose_count, &p,
      reinterpret_cast<vk_pose_score*>(score_poses_scores_.GetData()), score_poses_workspace_.GetData(), Device::GetStream()));
  std::vector<PoseScore> out(poses.size(), PoseScore{0, 0, 0, 0, 0, 0});
  if (count == 0) return out;                      // nothing was launched and nothing was written
  std::vector<vk_pose_score> scores(poses.size());
  score_poses_scores_.CopyToHost(reinterpret_cast<unsigned char*>(scores.data()));
  for (size_t k = 0; k < poses.size(); ++k)
    out[k] = PoseScore{scores[k].measured, scores[k].sampled, scores[k].residuals, scores[k].invalid, (long long)scores[k].sum_abs,
        (long long)scores[k].sum_squares};
  return out;
}

Localization Volume::LocalizeRays(const Ray* rays_dev, const float* ranges_dev, int count, const std::vector<Transform>& poses,
    int min_residuals, const RegisterRaysOptions& options) const
{
  vk_score_poses_params sp;
  sp.flags = RayFlags(options.voxel_units);
  sp.min_residuals = min_residuals;
  sp.r_min = options.r_min;
  sp.r_max = options.r_max;
  sp.max_abs_distance = options.max_abs_distance;
  sp.pad = 0;
  vk_register_rays_params p;
  p.flags = sp.flags;
  p.iterations = options.iterations;
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.max_abs_distance = options.max_abs_distance;
  p.pad = 0;
  const int pose_count = ScorePosesBuffers(count, poses);
  const size_t bytes = vk_volume_register_rays_workspace_bytes(count);
  if (bytes != 0 && register_rays_workspace_.GetSize() != bytes) register_rays_workspace_.Resize(bytes);
  if (score_poses_best_.GetSize() == 0) score_poses_best_.Resize(1);
  RegistrationBuffers& b = register_rays_;
  Localization out = {};
  out.best_index = -1;
  const float* rays = reinterpret_cast<const float*>(rays_dev);
  const vk_transform* candidates = reinterpret_cast<const vk_transform*>(score_poses_poses_.GetData());
  vk_pose_score* scores = reinterpret_cast<vk_pose_score*>(score_poses_scores_.GetData());
  const Transform identity;
  const vk_volume v = ToVk();
  // score, choose, refine: one enqueue. The identity stands in the pose buffer for the case that nothing is chosen
  b.Begin(count > 0 ? &identity : nullptr);        // no rays: no upload
  VK_ASSERT(vk_volume_score_poses(&v, rays, ranges_dev, count, candidates, pose_count, &sp, scores, score_poses_workspace_.GetData(),
      Device::GetStream()));
  if (count == 0) return out;                      // nothing was launched and nothing was written
  VK_ASSERT(vk_volume_score_poses_best(scores, candidates, pose_count, &sp, score_poses_best_.GetData(), b.pose, Device::GetStream()));
  VK_ASSERT(vk_volume_register_rays(&v, rays, ranges_dev, count, b.pose, &p, b.system, b.state, b.counts, b.update,
      register_rays_workspace_.GetData(), Device::GetStream()));
  score_poses_best_.CopyToHost(&out.best_index);
  if (out.best_index < 0) return out;              // what the loop refined from the identity is not a result
  static_cast<Registration&>(out) = b.Read();
  return out;
}

void Volume::Sample(const Vector3f* points_dev, int count, Voxel* samples_dev, Vector4f* gradients_dev, const Transform* pose,
    const SampleOptions& options) const
{
  vk_sample_params p;
  p.flags = (options.voxel_units ? VK_SAMPLE_VOXEL_UNITS : 0) | (options.distance_only ? VK_SAMPLE_DISTANCE_ONLY : 0);
  p.pad = 0;
  const vk_transform* pose_dev = PoseOnDevice(pose);
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_sample(&v, reinterpret_cast<const float*>(points_dev), count, pose_dev, &p, reinterpret_cast<vk_voxel*>(samples_dev),
      reinterpret_cast<float*>(gradients_dev), Device::GetStream()));
}

static vk_cell_grid ToVkGrid(const CellGrid& grid)
{
  vk_cell_grid g;
  for (int a = 0; a < 3; ++a)
  {
    g.origin[a] = grid.origin[a];
    g.dims[a] = grid.dims[a];
  }
  g.stride = grid.stride;
  g.pad = 0;
  return g;
}

void Volume::ClassifyCells(const CellGrid& grid, float occupied_below, Buffer<unsigned char>& classes) const
{
  const vk_cell_grid g = ToVkGrid(grid);
  VULCAN_ASSERT_MSG(vk_grid_distance_transform_workspace_bytes(g.dims) != 0, "a grid has 1 .. 1024 cells per axis and at most 2^27");
  if (classes.GetSize() != grid.Cells()) classes.Resize(grid.Cells());
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_classify_cells(&v, &g, occupied_below, classes.GetData(), Device::GetStream()));
}

void Volume::DistanceField(const CellGrid& grid, const DistanceFieldOptions& options, DistanceFieldBuffers& buffers) const
{
  const vk_cell_grid g = ToVkGrid(grid);
  vk_distance_field_params p;
  p.flags = options.is_signed ? VK_FIELD_SIGNED : 0;
  p.site_mask = options.site_mask;
  p.max_cells = options.max_cells;
  p.occupied_below = options.occupied_below;
  const size_t bytes = vk_volume_distance_field_workspace_bytes(&g, &p);
  VULCAN_ASSERT_MSG(bytes != 0, "a grid or options that vk_volume_distance_field refuses");
  const size_t cells = grid.Cells();
  if (field_workspace_.GetSize() != bytes) field_workspace_.Resize(bytes);
  if (buffers.classes.GetSize() != cells) buffers.classes.Resize(cells);
  if (buffers.distance.GetSize() != cells) buffers.distance.Resize(cells);
  if (options.squared && buffers.squared_cells.GetSize() != cells) buffers.squared_cells.Resize(cells);
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_distance_field(&v, &g, &p, buffers.classes.GetData(), options.squared ? buffers.squared_cells.GetData() : nullptr,
      buffers.distance.GetData(), field_workspace_.GetData(), Device::GetStream()));
}

void Volume::CastRays(const Ray* rays_dev, int count, float* t_dev, int* status_dev, Voxel* samples_dev, Vector4f* gradients_dev,
    const Transform* pose, const CastOptions& options) const
{
  static_assert(sizeof(Ray) == 6 * sizeof(float), "Ray layout");
  vk_cast_params p;
  p.flags = (options.voxel_units ? VK_CAST_VOXEL_UNITS : 0) | (options.distance_only ? VK_CAST_DISTANCE_ONLY : 0);
  p.max_steps = options.max_steps;
  p.t_min = options.t_min;
  p.t_max = options.t_max;
  const vk_transform* pose_dev = PoseOnDevice(pose);
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_cast_rays(&v, reinterpret_cast<const float*>(rays_dev), count, pose_dev, &p, t_dev, status_dev,
      reinterpret_cast<vk_voxel*>(samples_dev), reinterpret_cast<float*>(gradients_dev), Device::GetStream()));
}

IntegrateRaysCounts Volume::IntegrateRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform* pose,
    const IntegrateRaysOptions& options)
{
  static_assert(sizeof(Ray) == 6 * sizeof(float), "Ray layout");
  AssertNoFrameAnnounced();
  IntegrateRaysCounts out = {};
  vk_integrate_rays_params p;
  p.flags = RayFlags(options.voxel_units, options.one_observation);
  p.max_rounds = options.max_rounds;
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.max_distance_weight = options.max_distance_weight;
  p.pad = 0;
  Sized(rays_workspace_, vk_volume_integrate_rays_workspace_bytes(main_block_count_, excess_block_count_), rays_counts_);
  const vk_transform* pose_dev = PoseOnDevice(count > 0 ? pose : nullptr);      // no rays: no upload
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_integrate_rays(&v, reinterpret_cast<const float*>(rays_dev), ranges_dev, count, pose_dev, &p, rays_counts_.GetData(),
      rays_workspace_.GetData(), Device::GetStream()));
  if (count == 0) return out;                      // nothing was launched and the counts were not written
  VoidMadeAhead();
  const std::array<int32_t, 8> counts = EightCounts(rays_counts_);
  out.integrated = counts[0];
  out.unmeasured = counts[1];
  out.invalid = counts[2];
  out.allocated = counts[3];
  out.rounds = counts[4];
  out.blocks = counts[5];
  out.voxels = counts[6];
  out.lost = counts[7];
  int32_t counters[VK_CTR_PUBLIC];
  GetCounters(counters);
  NotePoolExhaustion(counters[VK_CTR_DROPPED]);
  EmptyVisibleList();
  return out;
}

CarveRaysCounts Volume::CarveRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform* pose,
    const CarveRaysOptions& options)
{
  static_assert(sizeof(Ray) == 6 * sizeof(float), "Ray layout");
  AssertNoFrameAnnounced();
  CarveRaysCounts out = {};
  vk_carve_rays_params p;
  p.flags = RayFlags(options.voxel_units, options.one_observation);
  p.max_blocks = options.max_blocks;
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.t_from = options.t_from;
  p.max_distance_weight = options.max_distance_weight;
  Sized(carve_workspace_, vk_volume_carve_rays_workspace_bytes(main_block_count_, excess_block_count_), carve_counts_);
  const vk_transform* pose_dev = PoseOnDevice(count > 0 ? pose : nullptr);      // no rays: no upload
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_carve_rays(&v, reinterpret_cast<const float*>(rays_dev), ranges_dev, count, pose_dev, &p, carve_counts_.GetData(),
      carve_workspace_.GetData(), Device::GetStream()));
  if (count == 0) return out;                      // nothing was launched and the counts were not written
  // the table and the visible list are as they were: nothing made ahead is void
  const std::array<int32_t, 8> counts = EightCounts(carve_counts_);
  out.carved = counts[0];
  out.nothing = counts[1];
  out.unmeasured = counts[2];
  out.invalid = counts[3];
  out.cut_short = counts[4];
  out.blocks = counts[5];
  out.voxels = counts[6];
  out.carves = unsigned(counts[7]);
  return out;
}

ColorRaysCounts Volume::ColorRays(const Ray* rays_dev, const float* ranges_dev, const Vector3f* colors_dev, int count,
    const Transform* pose, const ColorRaysOptions& options)
{
  static_assert(sizeof(Ray) == 6 * sizeof(float) && sizeof(Vector3f) == 3 * sizeof(float), "Ray and colour layout");
  AssertNoFrameAnnounced();
  ColorRaysCounts out = {};
  const vk_volume v = ToVk();
  vk_color_rays_params p;
  p.flags = RayFlags(options.voxel_units, options.one_observation);
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.band = options.band != 0.0f ? options.band : (options.voxel_units ? v.truncation_length / v.voxel_length : v.truncation_length);
  p.max_color_weight = options.max_color_weight;
  p.pad = 0;
  Sized(color_rays_workspace_, vk_volume_color_rays_workspace_bytes(main_block_count_, excess_block_count_), color_rays_counts_);
  const vk_transform* pose_dev = PoseOnDevice(count > 0 ? pose : nullptr);      // no rays: no upload
  VK_ASSERT(vk_volume_color_rays(&v, reinterpret_cast<const float*>(rays_dev), ranges_dev, reinterpret_cast<const float*>(colors_dev),
      count, pose_dev, &p, color_rays_counts_.GetData(), color_rays_workspace_.GetData(), Device::GetStream()));
  if (count == 0) return out;                      // nothing was launched and the counts were not written
  // the table and the visible list are as they were: nothing made ahead is void
  const std::array<int32_t, 8> counts = EightCounts(color_rays_counts_);
  out.coloured = counts[0];
  out.colourless = counts[1];
  out.unmeasured = counts[2];
  out.invalid = counts[3];
  out.blocks = counts[4];
  out.voxels = counts[5];
  out.not_near = counts[6];
  out.lost = unsigned(counts[7]);
  return out;
}

Registration Volume::RegisterRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform& start,
    const RegisterRaysOptions& options) const
{
  static_assert(sizeof(Ray) == 6 * sizeof(float), "Ray layout");
  // the volume is only read: allowed while a frame is announced, like Sample and CastRays
  vk_register_rays_params p;
  p.flags = RayFlags(options.voxel_units);
  p.iterations = options.iterations;
  p.r_min = options.r_min;
  p.r_max = options.r_max;
  p.max_abs_distance = options.max_abs_distance;
  p.pad = 0;
  const size_t bytes = vk_volume_register_rays_workspace_bytes(count);
  if (bytes != 0 && register_rays_workspace_.GetSize() != bytes) register_rays_workspace_.Resize(bytes);
  RegistrationBuffers& b = register_rays_;
  b.Begin(count > 0 ? &start : nullptr);           // no rays: no upload
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_register_rays(&v, reinterpret_cast<const float*>(rays_dev), ranges_dev, count, b.pose, &p, b.system, b.state,
      b.counts, b.update, register_rays_workspace_.GetData(), Device::GetStream()));
  if (count > 0) return b.Read();
  Registration out = {};                           // nothing was launched and nothing was written
  out.pose = start;
  return out;
}

void Volume::ResetBlockVisibility()
{
  AssertNoFrameAnnounced();
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_reset_block_visibility(&v, Device::GetStream()));
}

void Volume::UpdateBlockVisibility(const Frame& frame)
{
  view_bounds_.valid = 0;
  const vk_volume v = ToVk();
  const vk_projection k = frame.depth_projection.ToVk();
  const vk_transform Tdw = frame.depth_to_world_transform.Inverse().ToVk();
  VK_ASSERT(vk_volume_update_block_visibility(&v, frame.depth_image->GetWidth(),
      frame.depth_image->GetHeight(), &k, &Tdw, Device::GetStream()));
  visible_blocks_.Resize(GetBufferSize());
  visible_count_stale_ = false;
}

void Volume::CreateAllocationRequests(const Frame& frame)
{
  AssertNoFrameAnnounced();
  const vk_volume v = ToVk();
  const vk_projection k = frame.depth_projection.ToVk();
  const vk_transform Twd = frame.depth_to_world_transform.ToVk();
  VK_ASSERT(vk_volume_create_allocation_requests(&v, frame.depth_image->GetData(),
      frame.depth_image->GetWidth(), frame.depth_image->GetHeight(), &k, &Twd, Device::GetStream()));
}

void Volume::HandleAllocationRequests()
{
  AssertNoFrameAnnounced();
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_handle_allocation_requests(&v, Device::GetStream()));
}

int Volume::GetBufferSize() const
{
  int32_t counters[VK_CTR_PUBLIC];
  GetCounters(counters);
  return counters[VK_CTR_VISIBLE];
}

void Volume::ResetBufferSize() const
{
  VK_ASSERT(vk_memset(const_cast<int*>(counters_.GetData()) + VK_CTR_VISIBLE, 0, sizeof(int),
      Device::GetStream()));
}

void Volume::Initialize()
{
  // this translation unit and libvk_hip.so must agree on the structs and on the size of the counters block (vk.h)
  VK_ASSERT(vk_abi_check(VK_ABI_VERSION, sizeof(vk_volume), sizeof(vk_frame), VK_CTR_COUNT));
  // sizes as in volume.cu:565-627
  voxels_.Resize(size_t(max_block_count_) * Block::voxel_count);
  hash_entries_.Resize(max_block_count_);
  free_voxel_blocks_.Resize(max_block_count_);
  allocation_types_.Resize(main_block_count_);
  allocation_blocks_.Resize(main_block_count_);
  block_visibility_.Resize(max_block_count_);
  visible_blocks_.Reserve(max_block_count_);
  counters_.Resize(VK_CTR_COUNT);
  const vk_volume v = ToVk();
  VK_ASSERT(vk_volume_initialize(&v, Device::GetStream()));
}

} // namespace vulcan
