// chain_replay.cpp — a chain of tests/map_life.py, written as files by tests/chain_files.py, made call by call THROUGH THE
// CLASSES (Volume, Tracer, DepthIntegrator, Extractor); the C ABI only moves bytes (vk_memcpy_*, vk_memset), as
// volume_test_support.h does. tests/test_gpu_chain_replay.py compares what this program writes with the CPU statements: the
// class layer keeps its own copy of the caller's side of every volume operation (tsdf_volume.cpp: cached workspaces, the one
// pose buffer, VoidMadeAhead / EmptyVisibleList, the VK_MERGE_CONTINUE loop), and only a chain on one volume shows it.
//
//   ./chain_replay DIR as-allocated|ones|noise
//
// reads DIR/volumes.txt, DIR/script.txt and the arrays they name (chain_script.h), and writes into DIR/out, per step <i>:
//   <i>.counts                       the counts the call returned, int32 (load: the blocks of the pack that was saved)
//   <i>.origins, <i>.voxels          pack_merge: the pack itself; <i>.map (load): the file PackedVolume::Save wrote
//   <i>.<array>                      what a read step returned, raw (tests/chain_files.py RETURNS)
//   <i>.loop, <i>.pose               Register / RegisterRays: steps, end code, the four counts (the class's own buffers), then
//                                    the Registration's steps, converged, overlap, residuals; the pose as a vk_transform
//   <i>.state.<volume>.<buffer>      behind the steps whose line names the volume in state=: the seven small buffers whole,
//                                    public_counters (Volume::GetCounters), written + blocks (the pool slots that are not as the
//                                    constructor leaves them, and their bytes), visible_size (GetVisibleBlocks().GetSize())
//
// One Tracer, one DepthIntegrator and one Extractor per volume are created on first use and kept, so that an integration
// makes the raycast bounds ahead and a raycast alone sees whether the operation in between voided them.
//
// "ones" / "noise": before every step but a frame step the buffers the coming call will ask for are sized as the class sizes
// them, then every workspace, pose, score and counts buffer of every object is overwritten (0xFF; a fixed-seed xorshift; the
// counts with 0x5A5A5A5A). The classes keep those buffers protected: the two classes below derive to reach them. The object
// Volume::Load hands out is a plain Volume: its buffers cannot be reached and stay as its own calls leave them.
//
// Exit status 0: every step made and written. 1: an exception or a failed read, with the step's index and line; nothing
// further is run. Nothing is retried and no process is started.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include <vulcan/vulcan.h>

#include "chain_script.h"

using namespace vulcan;

namespace
{

const int32_t kSentinel = 0x5A5A5A5A;

enum Fill { kAsAllocated, kOnes, kNoise };

struct Dirt
{
  Fill fill = kAsAllocated;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  std::vector<unsigned char> host;

  uint64_t Next()
  {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
  }

  void Bytes(void* device, size_t bytes)
  {
    if (!device || bytes == 0) return;
    if (fill == kOnes) { VK_ASSERT(vk_memset(device, 0xFF, bytes, Device::GetStream())); return; }
    host.resize((bytes + 7) / 8 * 8);
    for (size_t at = 0; at < host.size(); at += 8)
    {
      const uint64_t word = Next();
      std::memcpy(host.data() + at, &word, 8);
    }
    VK_ASSERT(vk_memcpy_h2d(device, host.data(), bytes, Device::GetStream()));
  }

  void Counts(int* device, size_t count)
  {
    if (!device || count == 0) return;
    const std::vector<int32_t> sentinel(count, kSentinel);
    VK_ASSERT(vk_memcpy_h2d(device, sentinel.data(), count * sizeof(int32_t), Device::GetStream()));
  }
};

template <typename T>
void Soil(Dirt& dirt, Buffer<T>& buffer) { dirt.Bytes(buffer.GetData(), buffer.GetSize() * sizeof(T)); }

void SoilCounts(Dirt& dirt, Buffer<int>& buffer) { dirt.Counts(buffer.GetData(), buffer.GetSize()); }

class ReplayVolume : public Volume
{
  public:
    ReplayVolume(int main_blocks, int excess_blocks) : Volume(main_blocks, excess_blocks) {}

    // the buffers the coming call will ask for, sized with the calls and by the rules of tsdf_volume.cpp: the call keeps them
    void Expect(const chain::Step& step, const Volume* other)
    {
      const std::string& op = step.operation;
      const int main = main_block_count_, excess = excess_block_count_;
      const bool posed = step.Has("pose") && !step.Nothing("pose");
      if (op == "integrate_rays") Sized(rays_workspace_, vk_volume_integrate_rays_workspace_bytes(main, excess), rays_counts_, 8);
      else if (op == "carve_rays") Sized(carve_workspace_, vk_volume_carve_rays_workspace_bytes(main, excess), carve_counts_, 8);
      else if (op == "color_rays") Sized(color_rays_workspace_, vk_volume_color_rays_workspace_bytes(main, excess), color_rays_counts_, 8);
      else if (op == "release_blocks")
      {
        if (release_counts_.GetSize() == 0)
        {
          release_workspace_.Resize(vk_volume_release_workspace_bytes(main, excess));
          release_counts_.Resize(4);
        }
      }
      else if (op == "merge")
        Sized(merge_workspace_, vk_volume_merge_workspace_bytes(other->GetMainBlockCount(), other->GetExcessBlockCount()), merge_counts_, 6);
      else if (op == "merge_posed")
        Sized(merge_pose_workspace_, vk_volume_merge_posed_workspace_bytes(other->GetMainBlockCount(), other->GetExcessBlockCount(),
            main, excess), merge_pose_counts_, 8);
      else if (op == "merge_resampled")
      {
        const int box = std::min(8, int(other->GetVoxelLength() / GetVoxelLength() * 1.7320508f) + 2);      // K of vk.h
        Sized(merge_resample_workspace_, vk_volume_merge_resampled_workspace_bytes(other->GetMainBlockCount(), other->GetExcessBlockCount(),
            main, excess, box), merge_resample_counts_, 8);
      }
      else if (op == "pack_merge")
        Sized(merge_packed_workspace_, vk_volume_merge_packed_workspace_bytes(step.Int("packed")), merge_packed_counts_, 6);
      else if (op == "distance_field")
      {
        vk_cell_grid g;
        std::memset(&g, 0, sizeof(g));
        const std::vector<std::string> origin = step.Names("origin"), dims = step.Names("dims");
        if (origin.size() != 3 || dims.size() != 3) throw chain::Error("a grid has three coordinates and three sizes");
        for (int a = 0; a < 3; ++a)
        {
          g.origin[a] = chain::Integer(origin[a]);
          g.dims[a] = chain::Integer(dims[a]);
        }
        g.stride = step.Int("stride");
        vk_distance_field_params p;
        p.flags = step.Flag("signed") ? VK_FIELD_SIGNED : 0;
        p.site_mask = step.Int("sites");
        p.max_cells = step.Int("max_cells");
        p.occupied_below = 0.0f;
        const size_t bytes = vk_volume_distance_field_workspace_bytes(&g, &p);
        if (bytes != 0 && field_workspace_.GetSize() != bytes) field_workspace_.Resize(bytes);
      }
      else if (op == "register_terms")
      {
        const size_t bytes = vk_volume_register_workspace_bytes(other->GetMainBlockCount(), other->GetExcessBlockCount());
        if (register_workspace_.GetSize() != bytes) register_workspace_.Resize(bytes);
        register_.Begin(nullptr);
      }
      else if (op == "register_rays_terms")
      {
        const size_t bytes = vk_volume_register_rays_workspace_bytes(step.Int("count"));
        if (bytes != 0 && register_rays_workspace_.GetSize() != bytes) register_rays_workspace_.Resize(bytes);
        register_rays_.Begin(nullptr);
      }
      else if (op == "score_poses")
      {
        const size_t poses = size_t(step.Int("pose_count"));
        const size_t bytes = vk_volume_score_poses_workspace_bytes(step.Int("count"), int(poses));
        if (bytes != 0 && score_poses_workspace_.GetSize() != bytes) score_poses_workspace_.Resize(bytes);
        if (score_poses_scores_.GetSize() != poses * sizeof(vk_pose_score))
        {
          score_poses_scores_.Resize(poses * sizeof(vk_pose_score));
          score_poses_poses_.Resize(poses * 32);
        }
      }
      if (posed && (op == "integrate_rays" || op == "carve_rays" || op == "color_rays") && sample_pose_.GetSize() == 0)
        sample_pose_.Resize(32);
    }

    // Pack of this volume is coming (pack_merge and load read their source through it)
    void ExpectPack()
    {
      if (pack_counts_.GetSize() == 0)
      {
        pack_workspace_.Resize(vk_volume_pack_workspace_bytes(main_block_count_, excess_block_count_));
        pack_counts_.Resize(4);
      }
    }

    void Overwrite(Dirt& dirt)
    {
      Soil(dirt, merge_resample_workspace_);
      Soil(dirt, merge_packed_workspace_);
      Soil(dirt, pack_workspace_);
      Soil(dirt, field_workspace_);
      SoilCounts(dirt, merge_resample_counts_);
      SoilCounts(dirt, merge_packed_counts_);
      SoilCounts(dirt, pack_counts_);
      Soil(dirt, release_workspace_);
      Soil(dirt, merge_workspace_);
      Soil(dirt, merge_pose_workspace_);
      Soil(dirt, register_workspace_);
      Soil(dirt, register_.floats);
      Soil(dirt, sample_pose_);
      Soil(dirt, rays_workspace_);
      Soil(dirt, carve_workspace_);
      Soil(dirt, color_rays_workspace_);
      Soil(dirt, register_rays_workspace_);
      Soil(dirt, register_rays_.floats);
      Soil(dirt, score_poses_workspace_);
      Soil(dirt, score_poses_scores_);
      Soil(dirt, score_poses_poses_);
      SoilCounts(dirt, release_counts_);
      SoilCounts(dirt, merge_counts_);
      SoilCounts(dirt, merge_pose_counts_);
      SoilCounts(dirt, register_.ints);
      SoilCounts(dirt, rays_counts_);
      SoilCounts(dirt, carve_counts_);
      SoilCounts(dirt, color_rays_counts_);
      SoilCounts(dirt, register_rays_.ints);
      SoilCounts(dirt, score_poses_best_);
    }

    // the state (2) and the counts (4) a loop left in the class's own buffer
    void LoopInts(bool rays, int32_t* out) const
    {
      const Buffer<int>& ints = rays ? register_rays_.ints : register_.ints;
      VULCAN_ASSERT_MSG(ints.GetSize() == 6, "the loop left no state");
      ints.CopyToHost(out);
    }
};

class ReplayExtractor : public Extractor
{
  public:
    explicit ReplayExtractor(std::shared_ptr<const Volume> volume) : Extractor(volume) {}

    void Expect()
    {
      const vk_volume v = volume_->ToVk();
      const size_t bytes = vk_extract_workspace_bytes(v.main_block_count, v.excess_block_count);
      if (workspace_.GetSize() < bytes) workspace_.Resize(bytes);
    }

    void Overwrite(Dirt& dirt)
    {
      Soil(dirt, workspace_);
      SoilCounts(dirt, counts_);
    }
};

struct Kept
{
  chain::Shape shape;
  std::shared_ptr<Volume> volume;
  ReplayVolume* reach = nullptr;        // the same object where its protected buffers can be reached: not one Volume::Load made
  std::unique_ptr<DistanceFieldBuffers> field;      // the one set of output buffers DistanceField fills for this volume
  std::unique_ptr<Tracer> tracer;
  std::unique_ptr<DepthIntegrator> integrator;
  std::unique_ptr<ReplayExtractor> extractor;

  DistanceFieldBuffers& TheField()
  {
    if (!field) field.reset(new DistanceFieldBuffers());
    return *field;
  }
  Tracer& TheTracer()
  {
    if (!tracer) tracer.reset(new Tracer(volume));
    return *tracer;
  }
  DepthIntegrator& TheIntegrator()
  {
    if (!integrator) integrator.reset(new DepthIntegrator(volume));
    return *integrator;
  }
  ReplayExtractor& TheExtractor()
  {
    if (!extractor)
    {
      extractor.reset(new ReplayExtractor(volume));
      extractor->SetAllAllocated(true);
      extractor->SetInterpolate(true);
      extractor->SetColors(true);
      extractor->SetNormals(true);
    }
    return *extractor;
  }
};

struct Sizes
{
  size_t voxels, hash_entries, free_voxel_blocks, allocation_types, allocation_blocks, block_visibility, visible_blocks, counters;
  explicit Sizes(const vk_volume& v)
  {
    const size_t all = size_t(v.main_block_count) + size_t(v.excess_block_count), main = size_t(v.main_block_count);
    voxels = all * VK_BLOCK_VOXELS * sizeof(vk_voxel);
    hash_entries = all * sizeof(vk_hash_entry);
    free_voxel_blocks = all * sizeof(int32_t);
    allocation_types = main;
    allocation_blocks = main * sizeof(vk_block);
    block_visibility = all;
    visible_blocks = all * sizeof(int32_t);                  // (the class reserves the whole list)
    counters = size_t(VK_CTR_COUNT) * sizeof(int32_t);
  }
};

struct BufferOf { const char* name; void* device; size_t bytes; };

std::vector<BufferOf> Buffers(const Volume& volume)
{
  const vk_volume v = volume.ToVk();
  const Sizes s(v);
  return {{"voxels", v.voxels, s.voxels}, {"hash_entries", v.hash_entries, s.hash_entries},
      {"free_voxel_blocks", v.free_voxel_blocks, s.free_voxel_blocks}, {"allocation_types", v.allocation_types, s.allocation_types},
      {"allocation_blocks", v.allocation_blocks, s.allocation_blocks}, {"block_visibility", v.block_visibility, s.block_visibility},
      {"visible_blocks", v.visible_blocks, s.visible_blocks}, {"counters", v.counters, s.counters}};
}

std::shared_ptr<ReplayVolume> Construct(const chain::Shape& shape)
{
  auto volume = std::make_shared<ReplayVolume>(shape.main, shape.excess);
  volume->SetVoxelLength(shape.voxel_length);
  volume->SetTruncationLength(shape.truncation_length);
  volume->SetDepthRange(shape.depth_min, shape.depth_max);
  return volume;
}

class Replay
{
  public:
    Replay(const std::string& directory, Fill fill) : directory_(directory), out_(directory + "/out")
    {
      dirt_.fill = fill;
      ::mkdir(out_.c_str(), 0777);
      for (const chain::Shape& shape : chain::ReadVolumes(directory_))
      {
        Kept& kept = kept_[shape.name];
        kept.shape = shape;
        const std::shared_ptr<ReplayVolume> made = Construct(shape);
        kept.volume = made;
        kept.reach = made.get();
        // the counterpart of api.Volume.upload: the eight buffers as the files hold them, each of exactly the buffer's size
        for (const BufferOf& buffer : Buffers(*kept.volume))
        {
          const std::vector<unsigned char> host = chain::ReadFile(directory_ + "/" + shape.name + "." + buffer.name, buffer.bytes);
          VK_ASSERT(vk_memcpy_h2d(buffer.device, host.data(), buffer.bytes, Device::GetStream()));
        }
      }
      Device::Synchronize();
    }

    void Run(const chain::Step& step)
    {
      const std::string& op = step.operation;
      Kept& on = Of(step.Get("on"));
      const Volume* other = step.Has("source") ? Of(step.Get("source")).volume.get() : nullptr;
      if (dirt_.fill != kAsAllocated && op != "frame" && op != "second_volume")
      {
        if (on.reach) on.reach->Expect(step, other);
        if ((op == "pack_merge" || op == "load") && Of(step.Get("source")).reach) Of(step.Get("source")).reach->ExpectPack();
        if (op == "extract") on.TheExtractor().Expect();
        for (auto& entry : kept_)
        {
          if (entry.second.reach) entry.second.reach->Overwrite(dirt_);
          if (entry.second.extractor) entry.second.extractor->Overwrite(dirt_);
          Soil(dirt_, entry.second.TheField().classes);
          Soil(dirt_, entry.second.TheField().distance);
          Soil(dirt_, entry.second.TheField().squared_cells);
        }
      }
      if (op == "integrate_rays") IntegrateRays(step, on);
      else if (op == "color_rays") ColorRays(step, on);
      else if (op == "carve_rays") CarveRays(step, on);
      else if (op == "release_blocks") ReleaseBlocks(step, on);
      else if (op == "merge") Merge(step, on, *other);
      else if (op == "merge_posed") MergePosed(step, on, *other);
      else if (op == "merge_resampled") MergeResampled(step, on, *other);
      else if (op == "pack_merge") PackMerge(step, on, *other);
      else if (op == "load") Load(step, on, *other);
      else if (op == "distance_field") DistanceField(step, on);
      else if (op == "frame") FrameStep(step, on);
      else if (op == "raycast") Raycast(step, on);
      else if (op == "sample") Sample(step, on);
      else if (op == "cast_rays") CastRays(step, on);
      else if (op == "extract") Extract(step, on);
      else if (op == "score_poses") ScorePoses(step, on);
      else if (op == "register_terms") Register(step, on, *other);
      else if (op == "register_rays_terms") RegisterRays(step, on);
      else if (op == "second_volume") SecondVolume(on);
      else throw chain::Error("an operation the class layer has no call for: " + op);
      Device::Synchronize();
      for (const std::string& name : step.Names("state")) DumpState(step.index, name, *Of(name).volume);
    }

  private:
    std::string directory_, out_;
    Dirt dirt_;
    std::map<std::string, Kept> kept_;
    std::map<std::string, std::shared_ptr<Buffer<unsigned char>>> arrays_;

    Kept& Of(const std::string& name)
    {
      const auto found = kept_.find(name);
      if (found == kept_.end()) throw chain::Error("no volume '" + name + "'");
      return found->second;
    }

    // a file of exactly `bytes` bytes on the device, uploaded once
    const unsigned char* Array(const std::string& file, size_t bytes)
    {
      auto& held = arrays_[file];
      if (!held)
      {
        const std::vector<unsigned char> host = chain::ReadFile(directory_ + "/" + file, bytes);
        held = std::make_shared<Buffer<unsigned char>>(bytes);
        held->CopyFromHost(host.data());
      }
      if (held->GetSize() != bytes) throw chain::Error(file + " is read with two sizes");
      return held->GetData();
    }

    Transform PoseOf(const std::string& file) const
    {
      const std::vector<unsigned char> host = chain::ReadFile(directory_ + "/" + file, sizeof(vk_transform));
      vk_transform pose;
      std::memcpy(&pose, host.data(), sizeof(pose));
      return Transform::FromVk(pose);
    }

    // the pose of a step as the calls take it: null for "-"
    const Transform* Pose(const chain::Step& step, Transform& storage) const
    {
      if (step.Nothing("pose")) return nullptr;
      storage = PoseOf(step.Get("pose"));
      return &storage;
    }

    const Ray* Rays(const chain::Step& step) { return reinterpret_cast<const Ray*>(Array(step.Get("rays"), size_t(step.Int("count")) * sizeof(Ray))); }
    const float* Ranges(const chain::Step& step) { return reinterpret_cast<const float*>(Array(step.Get("ranges"), size_t(step.Int("count")) * sizeof(float))); }

    std::string Path(int index, const std::string& what) const { return out_ + "/" + std::to_string(index) + "." + what; }

    void Write(int index, const std::string& what, const void* data, size_t bytes) const { chain::WriteFile(Path(index, what), data, bytes); }

    void WriteDevice(int index, const std::string& what, const void* device, size_t bytes) const
    {
      std::vector<unsigned char> host(bytes);
      if (bytes) VK_ASSERT(vk_memcpy_d2h(host.data(), device, bytes, Device::GetStream()));
      Write(index, what, host.data(), bytes);
    }

    void IntegrateRays(const chain::Step& step, Kept& on)
    {
      IntegrateRaysOptions options;
      options.voxel_units = step.Flag("voxel_units");
      options.one_observation = step.Flag("one_observation");
      options.r_min = step.Float("r_min");
      options.r_max = step.Float("r_max");
      options.max_distance_weight = step.Float("cap");
      Transform storage;
      const IntegrateRaysCounts c = on.volume->IntegrateRays(Rays(step), Ranges(step), step.Int("count"), Pose(step, storage), options);
      const int32_t counts[8] = {c.integrated, c.unmeasured, c.invalid, c.allocated, c.rounds, c.blocks, c.voxels, c.lost};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void ColorRays(const chain::Step& step, Kept& on)
    {
      ColorRaysOptions options;
      options.voxel_units = step.Flag("voxel_units");
      options.one_observation = step.Flag("one_observation");
      options.r_min = step.Float("r_min");
      options.r_max = step.Float("r_max");
      options.band = step.Float("band");
      options.max_color_weight = step.Float("cap");
      const Vector3f* colors = reinterpret_cast<const Vector3f*>(Array(step.Get("colors"), size_t(step.Int("count")) * 3 * sizeof(float)));
      Transform storage;
      const ColorRaysCounts c = on.volume->ColorRays(Rays(step), Ranges(step), colors, step.Int("count"), Pose(step, storage), options);
      const int32_t counts[8] = {c.coloured, c.colourless, c.unmeasured, c.invalid, c.blocks, c.voxels, c.not_near, int32_t(c.lost)};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void CarveRays(const chain::Step& step, Kept& on)
    {
      CarveRaysOptions options;
      options.voxel_units = step.Flag("voxel_units");
      options.one_observation = step.Flag("one_observation");
      options.r_min = step.Float("r_min");
      options.r_max = step.Float("r_max");
      options.t_from = step.Float("t_from");
      options.max_distance_weight = step.Float("cap");
      Transform storage;
      const CarveRaysCounts c = on.volume->CarveRays(Rays(step), Ranges(step), step.Int("count"), Pose(step, storage), options);
      const int32_t counts[8] = {c.carved, c.nothing, c.unmeasured, c.invalid, c.cut_short, c.blocks, c.voxels, int32_t(c.carves)};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void ReleaseBlocks(const chain::Step& step, Kept& on)
    {
      ReleaseRule rule;
      rule.unobserved = step.Flag("unobserved");
      rule.no_surface = step.Flag("no_surface");
      rule.min_abs_distance = step.Float("min_abs_distance");
      rule.outside_box = step.Flag("outside_box");
      const std::vector<std::string> lo = step.Names("keep_lo"), hi = step.Names("keep_hi");
      if (lo.size() != 3 || hi.size() != 3) throw chain::Error("a box has three coordinates a corner");
      for (int a = 0; a < 3; ++a)
      {
        rule.keep_lo[a] = int16_t(chain::Integer(lo[a]));
        rule.keep_hi[a] = int16_t(chain::Integer(hi[a]));
      }
      const ReleaseCounts c = on.volume->ReleaseBlocks(rule);
      const int32_t counts[4] = {c.released, c.kept, c.excess_entries, c.free_slots};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void Merge(const chain::Step& step, Kept& on, const Volume& other)
    {
      MergeOptions options;
      options.max_rounds = step.Int("max_rounds");
      const MergeCounts c = on.volume->Merge(other, options);
      const int32_t counts[6] = {c.considered, c.fused, c.allocated, c.left_out, c.rounds, c.skipped};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void MergePosed(const chain::Step& step, Kept& on, const Volume& other)
    {
      MergeOptions options;
      options.max_rounds = step.Int("max_rounds");
      const MergePoseCounts c = on.volume->Merge(other, PoseOf(step.Get("pose")), options);
      const int32_t counts[8] = {c.considered, c.candidates, c.fused, c.allocated, c.left_out, c.rounds, c.skipped, c.sampled};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void MergeResampled(const chain::Step& step, Kept& on, const Volume& other)
    {
      MergeOptions options;
      options.max_rounds = step.Int("max_rounds");
      options.skip_unobserved = step.Flag("skip_unobserved");
      const MergePoseCounts c = on.volume->MergeResampled(other, PoseOf(step.Get("pose")), step.Int("supersample"), options);
      const int32_t counts[8] = {c.considered, c.candidates, c.fused, c.allocated, c.left_out, c.rounds, c.skipped, c.sampled};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void PackMerge(const chain::Step& step, Kept& on, const Volume& other)
    {
      PackOptions rule;
      rule.skip_unobserved = step.Flag("skip_unobserved");
      rule.box = step.Flag("box");
      const std::vector<std::string> lo = step.Names("lo"), hi = step.Names("hi");
      if (lo.size() != 3 || hi.size() != 3) throw chain::Error("a box has three coordinates a corner");
      for (int a = 0; a < 3; ++a)
      {
        rule.lo[a] = int16_t(chain::Integer(lo[a]));
        rule.hi[a] = int16_t(chain::Integer(hi[a]));
      }
      const PackedVolume pack = other.Pack(rule);
      MergeOptions options;
      options.max_rounds = step.Int("max_rounds");
      const MergeCounts c = on.volume->Merge(pack, options);
      const int32_t counts[6] = {c.considered, c.fused, c.allocated, c.left_out, c.rounds, c.skipped};
      Write(step.index, "counts", counts, sizeof(counts));
      WriteDevice(step.index, "origins", pack.GetOrigins().GetData(), size_t(pack.Count()) * 4 * sizeof(int16_t));
      WriteDevice(step.index, "voxels", pack.GetVoxels().GetData(), size_t(pack.Count()) * VK_BLOCK_VOXELS * sizeof(vk_voxel));
    }

    // the source packed whole and saved; the file loaded as a new Volume of the sizes of `on`, which takes its place
    void Load(const chain::Step& step, Kept& on, const Volume& other)
    {
      const PackedVolume pack = other.Pack();
      const std::string path = Path(step.index, "map");
      pack.Save(path);
      const std::shared_ptr<Volume> loaded = Volume::Load(path, on.shape.main, on.shape.excess);
      loaded->SetDepthRange(on.shape.depth_min, on.shape.depth_max);
      on.tracer.reset();
      on.integrator.reset();
      on.extractor.reset();
      on.volume = loaded;
      on.reach = nullptr;
      on.field.reset();
      const int32_t counts[1] = {pack.Count()};
      Write(step.index, "counts", counts, sizeof(counts));
    }

    void DistanceField(const chain::Step& step, Kept& on)
    {
      CellGrid grid;
      const std::vector<std::string> origin = step.Names("origin"), dims = step.Names("dims");
      if (origin.size() != 3 || dims.size() != 3) throw chain::Error("a grid has three coordinates and three sizes");
      for (int a = 0; a < 3; ++a)
      {
        grid.origin[a] = chain::Integer(origin[a]);
        grid.dims[a] = chain::Integer(dims[a]);
      }
      grid.stride = step.Int("stride");
      DistanceFieldOptions options;
      options.site_mask = step.Int("sites");
      options.max_cells = step.Int("max_cells");
      options.is_signed = step.Flag("signed");
      options.squared = true;
      const Volume& volume = *on.volume;                 // DistanceField is const: field_workspace_ is resized behind it
      DistanceFieldBuffers& field = on.TheField();
      volume.DistanceField(grid, options, field);
      const size_t cells = grid.Cells();
      if (field.classes.GetSize() != cells || field.distance.GetSize() != cells || field.squared_cells.GetSize() != cells)
        throw chain::Error("the field's buffers are not of the grid's size");
      WriteDevice(step.index, "classes", field.classes.GetData(), cells);
      WriteDevice(step.index, "squared_cells", field.squared_cells.GetData(), cells * sizeof(int));
      WriteDevice(step.index, "distance", field.distance.GetData(), cells * sizeof(float));
    }

    // the frame a raycast fills: the camera of the step, images of its size
    Frame Target(const chain::Step& step) const
    {
      const std::vector<unsigned char> k = chain::ReadFile(directory_ + "/" + step.Get("projection"), 4 * sizeof(float));
      float f[4];
      std::memcpy(f, k.data(), sizeof(f));
      Frame frame;
      frame.depth_projection.SetFocalLength(f[0], f[1]);
      frame.depth_projection.SetCenterPoint(f[2], f[3]);
      frame.depth_to_world_transform = PoseOf(step.Get("pose"));
      return frame;
    }

    void Images(const chain::Step& step, const Frame& frame) const
    {
      WriteDevice(step.index, "depth", static_cast<const Image&>(*frame.depth_image).GetData(), size_t(frame.depth_image->GetBytes()));
      WriteDevice(step.index, "color", static_cast<const ColorImage&>(*frame.color_image).GetData(), size_t(frame.color_image->GetBytes()));
      WriteDevice(step.index, "normals", static_cast<const ColorImage&>(*frame.normal_image).GetData(), size_t(frame.normal_image->GetBytes()));
    }

    void Trace(const chain::Step& step, Kept& on)
    {
      Frame out = Target(step);
      out.Allocate(step.Int("width"), step.Int("height"));
      on.TheTracer().Trace(out);
      Images(step, out);
    }

    void FrameStep(const chain::Step& step, Kept& on)
    {
      const int w = step.Int("width"), h = step.Int("height");
      if (w <= 0 || h <= 0 || w > 4096 || h > 4096) throw chain::Error("a frame of no size");
      Frame frame = Target(step);
      const std::vector<unsigned char> depth = chain::ReadFile(directory_ + "/" + step.Get("depth"), size_t(w) * h * sizeof(float));
      frame.depth_image = std::make_shared<Image>(w, h);
      frame.depth_image->CopyFromHost(reinterpret_cast<const float*>(depth.data()));
      // vk_volume_set_view_rounds ends its rounds with the first that drops a request (vk.h): where the statement's three
      // calls dropped one, three calls
      if (step.Flag("ran_dry"))
        for (int round = 0; round < 3; ++round) on.volume->SetView(frame);
      else
        on.volume->SetView(frame, 3);
      on.TheTracer();                                  // attached before the integration: its bounds are made ahead
      on.TheIntegrator().Integrate(frame);
      Trace(step, on);
    }

    void Raycast(const chain::Step& step, Kept& on)
    {
      const int w = step.Int("width"), h = step.Int("height");
      if (w <= 0 || h <= 0 || w > 4096 || h > 4096) throw chain::Error("a frame of no size");
      Trace(step, on);
    }

    void Sample(const chain::Step& step, Kept& on)
    {
      const size_t count = size_t(step.Int("count"));
      const Vector3f* points = reinterpret_cast<const Vector3f*>(Array(step.Get("points"), count * 3 * sizeof(float)));
      Buffer<unsigned char> samples(count * sizeof(vk_voxel)), gradients(count * 4 * sizeof(float));
      SampleOptions options;
      options.voxel_units = true;
      on.volume->Sample(points, int(count), reinterpret_cast<Voxel*>(samples.GetData()), reinterpret_cast<Vector4f*>(gradients.GetData()),
          nullptr, options);
      WriteDevice(step.index, "samples", samples.GetData(), samples.GetSize());
      WriteDevice(step.index, "gradients", gradients.GetData(), gradients.GetSize());
    }

    void CastRays(const chain::Step& step, Kept& on)
    {
      const size_t count = size_t(step.Int("count"));
      Buffer<unsigned char> samples(count * sizeof(vk_voxel)), gradients(count * 4 * sizeof(float));
      Buffer<float> t(count);
      Buffer<int> status(count);
      CastOptions options;
      options.t_max = step.Float("t_max");
      options.max_steps = step.Int("max_steps");
      on.volume->CastRays(Rays(step), int(count), t.GetData(), status.GetData(), reinterpret_cast<Voxel*>(samples.GetData()),
          reinterpret_cast<Vector4f*>(gradients.GetData()), nullptr, options);
      WriteDevice(step.index, "status", status.GetData(), count * sizeof(int));
      WriteDevice(step.index, "t", t.GetData(), count * sizeof(float));
      WriteDevice(step.index, "samples", samples.GetData(), samples.GetSize());
      WriteDevice(step.index, "gradients", gradients.GetData(), gradients.GetSize());
    }

    void Extract(const chain::Step& step, Kept& on)
    {
      Mesh mesh;
      on.TheExtractor().Extract(mesh);
      Write(step.index, "points", mesh.points.data(), mesh.points.size() * sizeof(Vector3f));
      Write(step.index, "faces", mesh.faces.data(), mesh.faces.size() * sizeof(Vector3i));
      Write(step.index, "colors", mesh.colors.data(), mesh.colors.size() * sizeof(Vector3f));
      Write(step.index, "normals", mesh.normals.data(), mesh.normals.size() * sizeof(Vector3f));
    }

    void ScorePoses(const chain::Step& step, Kept& on)
    {
      const size_t pose_count = size_t(step.Int("pose_count"));
      const std::vector<unsigned char> host = chain::ReadFile(directory_ + "/" + step.Get("poses"), pose_count * sizeof(vk_transform));
      std::vector<Transform> poses;
      for (size_t k = 0; k < pose_count; ++k)
      {
        vk_transform pose;
        std::memcpy(&pose, host.data() + k * sizeof(pose), sizeof(pose));
        poses.push_back(Transform::FromVk(pose));
      }
      ScorePosesOptions options;
      options.r_min = step.Float("r_min");
      options.r_max = step.Float("r_max");
      options.max_abs_distance = step.Float("band");
      const std::vector<PoseScore> scores = on.volume->ScorePoses(Rays(step), Ranges(step), step.Int("count"), poses, options);
      std::vector<vk_pose_score> raw(scores.size());
      std::memset(raw.data(), 0, raw.size() * sizeof(vk_pose_score));
      for (size_t k = 0; k < scores.size(); ++k)
      {
        raw[k].measured = scores[k].measured;
        raw[k].sampled = scores[k].sampled;
        raw[k].residuals = scores[k].residuals;
        raw[k].invalid = scores[k].invalid;
        raw[k].sum_abs = scores[k].sum_abs;
        raw[k].sum_squares = scores[k].sum_squares;
      }
      Write(step.index, "scores", raw.data(), raw.size() * sizeof(vk_pose_score));
    }

    void Loop(const chain::Step& step, Kept& on, bool rays, const Registration& result)
    {
      int32_t ints[10];
      if (!on.reach) throw chain::Error("the loop's own buffers of a loaded volume cannot be reached");
      on.reach->LoopInts(rays, ints);
      ints[6] = result.steps;
      ints[7] = result.converged ? 1 : 0;
      ints[8] = result.overlap ? 1 : 0;
      ints[9] = result.residuals;
      Write(step.index, "loop", ints, sizeof(ints));
      const vk_transform pose = result.pose.ToVk();
      Write(step.index, "pose", &pose, sizeof(pose));
    }

    void Register(const chain::Step& step, Kept& on, const Volume& other)
    {
      Loop(step, on, false, on.volume->Register(other, PoseOf(step.Get("pose")), step.Int("iterations"), step.Float("band")));
    }

    void RegisterRays(const chain::Step& step, Kept& on)
    {
      RegisterRaysOptions options;
      options.iterations = step.Int("iterations");
      options.r_min = step.Float("r_min");
      options.r_max = step.Float("r_max");
      options.max_abs_distance = step.Float("band");
      Loop(step, on, true, on.volume->RegisterRays(Rays(step), Ranges(step), step.Int("count"), PoseOf(step.Get("pose")), options));
    }

    // a second Volume object takes the eight buffers, device to device, and the first one's place: it has made no call
    void SecondVolume(Kept& on)
    {
      std::shared_ptr<ReplayVolume> second = Construct(on.shape);
      const std::vector<BufferOf> from = Buffers(*on.volume), to = Buffers(*second);
      for (size_t k = 0; k < from.size(); ++k)
        VK_ASSERT(vk_memcpy_d2d(to[k].device, from[k].device, from[k].bytes, Device::GetStream()));
      Device::Synchronize();
      on.tracer.reset();
      on.integrator.reset();
      on.extractor.reset();
      on.volume = second;
      on.reach = second.get();
      on.field.reset();
    }

    void DumpState(int index, const std::string& name, const Volume& volume) const
    {
      const std::string prefix = "state." + name + ".";
      std::vector<unsigned char> voxels;
      for (const BufferOf& buffer : Buffers(volume))
      {
        std::vector<unsigned char> host(buffer.bytes);
        VK_ASSERT(vk_memcpy_d2h(host.data(), buffer.device, buffer.bytes, Device::GetStream()));
        if (std::string(buffer.name) == "voxels") voxels.swap(host);
        else Write(index, prefix + buffer.name, host.data(), host.size());
      }
      int32_t counters[VK_CTR_PUBLIC];
      volume.GetCounters(counters);
      Write(index, prefix + "public_counters", counters, sizeof(counters));
      // the blocks that are not as the constructor leaves them (distance 1, everything else 0)
      const size_t block_bytes = size_t(VK_BLOCK_VOXELS) * sizeof(vk_voxel), blocks = voxels.size() / block_bytes;
      std::vector<unsigned char> empty(block_bytes, 0);
      const float one = 1.0f;
      for (size_t i = 0; i < VK_BLOCK_VOXELS; ++i) std::memcpy(empty.data() + i * sizeof(vk_voxel) + offsetof(vk_voxel, distance), &one, sizeof(one));
      std::vector<int32_t> written;
      std::vector<unsigned char> bytes;
      for (size_t slot = 0; slot < blocks; ++slot)
      {
        const unsigned char* block = voxels.data() + slot * block_bytes;
        if (std::memcmp(block, empty.data(), block_bytes) == 0) continue;
        written.push_back(int32_t(slot));
        bytes.insert(bytes.end(), block, block + block_bytes);
      }
      Write(index, prefix + "written", written.data(), written.size() * sizeof(int32_t));
      Write(index, prefix + "blocks", bytes.data(), bytes.size());
      const int32_t visible = int32_t(volume.GetVisibleBlocks().GetSize());
      Write(index, prefix + "visible_size", &visible, sizeof(visible));
    }
};

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: %s DIR as-allocated|ones|noise\n", argv[0]);
    return 2;
  }
  const std::string how = argv[2];
  if (how != "as-allocated" && how != "ones" && how != "noise")
  {
    std::fprintf(stderr, "chain_replay: the fill is as-allocated, ones or noise, not '%s'\n", how.c_str());
    return 2;
  }
  const Fill fill = how == "ones" ? kOnes : how == "noise" ? kNoise : kAsAllocated;
  int index = -1;
  std::string text = "(reading the script and the start volumes)";
  try
  {
    int devices = 0;
    VK_ASSERT(vk_device_count(&devices));
    if (devices == 0) throw chain::Error("no HIP device");
    const std::vector<chain::Step> steps = chain::ReadScript(argv[1]);
    Replay replay(argv[1], fill);
    for (const chain::Step& step : steps)
    {
      index = step.index;
      text = step.text;
      replay.Run(step);
      std::printf("step %d %s\n", step.index, step.operation.c_str());
      std::fflush(stdout);
    }
    Device::Synchronize();
  }
  catch (const std::exception& error)
  {
    std::printf("chain_replay: step %d failed: %s\n  %s\n", index, error.what(), text.c_str());
    return 1;
  }
  std::printf("chain_replay: %s, fill %s: every step made and written\n", argv[1], how.c_str());
  return 0;
}
