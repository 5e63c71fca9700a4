// tsdf_volume.h — the voxel-hashed TSDF volume and the per-entry flag enums.
//
// API parity: class Volume keeps the public AND protected surface of the
// reference's volume.h:16-117 (its tests subclass Volume to reach the four
// SetView stages, tests/volume_test.cpp:23-31); Visibility / AllocationType
// keep the values of types.h. Both header names remain as forwarders.
// What differs behind the names:
//   * the device counters (visible count, free-slot pointer, excess pointer)
//     live in a per-volume buffer instead of process-wide __device__ symbols
//     (volume.cu:17-21), so one process can hold several volumes;
//   * SetView never blocks; the visible count is read back lazily by the first
//     GetVisibleBlocks() after it (volume.cu:494 synchronised every frame).
#pragma once

#include <cmath>
#include <cstdint>
#include <array>
#include <memory>
#include <string>
#include <vector>
#include <vk.h>
#include <vulcan/buffer.h>
#include <vulcan/matrix.h>
#include <vulcan/transform.h>

namespace vulcan
{

// per hash entry: was the block seen by the current view
enum Visibility : uint8_t
{
  VISIBILITY_UNKNOWN = 0,
  VISIBILITY_FALSE   = 1,
  VISIBILITY_TRUE    = 2,
};

// per hash entry: what kind of allocation the current view requested there
enum AllocationType : uint8_t
{
  ALLOC_TYPE_NONE   = 0,
  ALLOC_TYPE_MAIN   = 1,
  ALLOC_TYPE_EXCESS = 2,
};

// Not upstream: which blocks Volume::ReleaseBlocks gives back (vk_release_rule). A default-constructed rule releases
// nothing: the call is then the repair alone.
struct ReleaseRule
{
  bool unobserved = false;            // no voxel of the block was ever integrated
  bool no_surface = false;            // observed, but no observed voxel's stored distance is below min_abs_distance
  float min_abs_distance = 0.0f;      //   (stored distances are normalised to (-1, 1])
  bool outside_box = false;           // the block's origin lies outside [keep_lo, keep_hi], block coordinates, inclusive
  int16_t keep_lo[3] = {0, 0, 0};
  int16_t keep_hi[3] = {0, 0, 0};
};

struct ReleaseCounts
{
  int released;         // blocks given back by this call
  int kept;             // blocks in the volume afterwards
  int excess_entries;   // excess hash entries in use afterwards
  int free_slots;       // pool slots free afterwards
};

// Not upstream: how Volume::Merge fuses another volume into this one (vk_merge_params)
struct MergeOptions
{
  float max_distance_weight = 16.0f;  // the caps an integrator would apply (integrator.cu:7-13)
  float max_color_weight = 16.0f;
  bool skip_unobserved = false;       // leave out the source blocks no voxel of which was ever integrated
  int max_rounds = 8;                 // allocation rounds per call of vk_volume_merge
};

struct MergeCounts
{
  int considered;       // blocks of the other volume the merge looked at
  int fused;            // of those, fused into this volume
  int allocated;        // blocks this volume did not have before
  int left_out;         // blocks that found no room: the pool or the excess list ran out
  int rounds;           // allocation rounds that posted a request
  int skipped;          // blocks of the other volume skipped as unobserved
};

// Not upstream: which blocks Volume::Pack leaves out (vk_pack_rule). Default-constructed: every block.
struct PackOptions
{
  bool skip_unobserved = false;       // without the blocks no voxel of which was ever integrated
  bool box = false;                   // only the blocks whose origin lies in [lo, hi], block coordinates, inclusive
  int16_t lo[3] = {0, 0, 0};
  int16_t hi[3] = {0, 0, 0};
};

// Not upstream (its Volume never leaves the device buffers it was allocated in, src/volume.cu:17-21): the blocks of a
// volume, compact and in a defined order (vk_block_pack) — per block its origin (x, y, z, 0) and its 10 240 bytes of
// voxels, in ascending order of the blocks' table entries. What Volume::Pack returns and Volume::Merge takes in a volume's
// place; Save and Load move it through a file, at the size of its blocks. Copies share the two device buffers.
class PackedVolume
{
  public:
    PackedVolume();                                 // no blocks
    int Count() const { return count_; }
    float VoxelLength() const { return voxel_length_; }
    float TruncationLength() const { return truncation_length_; }
    const Buffer<int16_t>& GetOrigins() const { return *origins_; }           // device [4 * Count()]
    const Buffer<unsigned char>& GetVoxels() const { return *voxels_; }       // device [10240 * Count()]
    vk_block_pack ToVk() const;                     // device view for the C ABI
    // The file of vulcan_amd/io.py write_map / read_map, little-endian: the magic "VULCANMP", int32 version 1, int32 block
    // count, float voxel length, float truncation length, 8 reserved bytes (zero), the origins, the voxels. Blocking.
    void Save(const std::string& path) const;
    // Throws for a file that is not one — a wrong magic or version, a negative count, a length that does not match the
    // count, a fourth origin component that is not 0, two blocks with one origin — before anything reaches the device.
    static PackedVolume Load(const std::string& path);

  private:
    friend class Volume;
    PackedVolume(int count, float voxel_length, float truncation_length);     // device buffers for `count` blocks
    std::shared_ptr<Buffer<int16_t>> origins_;
    std::shared_ptr<Buffer<unsigned char>> voxels_;
    int count_;
    float voxel_length_, truncation_length_;
};

// Volume::Merge through a pose (vk_volume_merge_posed's eight counts, summed over the calls the rounds take)
struct MergePoseCounts
{
  int considered;       // blocks of the other volume the merge looked at
  int candidates;       // blocks of this volume those reach through the pose
  int fused;            // of those, sampled into
  int allocated;        // blocks this volume did not have before
  int left_out;         // candidates that found no room: the pool or the excess list ran out
  int rounds;           // allocation rounds that posted a request
  int skipped;          // blocks of the other volume skipped as unobserved
  int sampled;          // voxels that took a distance sample
};

// Volume::Register (vk_volume_register) and Volume::RegisterRays (vk_volume_register_rays)
struct Registration
{
  Transform pose;       // Tdst_src after the last step: what Merge(other, pose) takes; RegisterRays: Tvolume_rays, IntegrateRays' pose
  int steps;            // Gauss-Newton steps run
  bool converged;       // the last step was shorter than 1e-6
  bool overlap;         // false: a step found no voxel (no return) to compare; the pose is the one it had then
  int residuals;        // voxels (returns) compared in the last evaluated step
  float rms;            // sqrt(sum r^2 / residuals) of that step, in truncation lengths
};

// Not upstream: how Volume::Sample reads its points and what it samples (vk_sample_params)
struct SampleOptions
{
  bool voxel_units = false;     // the points are in voxels, not metres: a voxel's centre is then exactly representable
  bool distance_only = false;   // the colour fields of a sample stay 0 and no colour is read
};

// Not upstream: a dense grid of cells over the volume's lattice (vk_cell_grid): cell (i, j, k) covers the stride^3 voxels from
// origin + stride * (i, j, k); arrays over it are indexed (k * ny + j) * nx + i
struct CellGrid
{
  int origin[3] = {0, 0, 0};    // lattice coordinates of the first voxel, each a multiple of stride
  int dims[3] = {1, 1, 1};      // cells per axis (nx, ny, nz): 1 .. 1024 each, 2^27 in all
  int stride = 1;               // voxels per cell and axis: 1, 2, 4 or 8
  size_t Cells() const { return size_t(dims[0]) * size_t(dims[1]) * size_t(dims[2]); }
};

// Not upstream: what Volume::DistanceField measures (vk_distance_field_params)
struct DistanceFieldOptions
{
  int site_mask = VK_CELL_OCCUPIED;   // the classes a distance is measured to, VK_CELL_* or'ed
  int max_cells = 256;                // the cap of the search, in cells (1 .. 256); beyond it the distance is +infinity
  float occupied_below = 0.0f;        // an observed voxel is occupied where its stored distance is <= this, truncation lengths
  bool is_signed = false;             // a site cell takes minus its distance to the nearest cell that is no site
  bool squared = false;               // also the squared distance in cells (int32, VK_FIELD_BEYOND beyond the cap)
};

// Not upstream: the device buffers Volume::DistanceField and ClassifyCells fill, one element per cell: allocated by the first
// call, again for a grid of another size
struct DistanceFieldBuffers
{
  Buffer<unsigned char> classes;      // VK_CELL_UNKNOWN, VK_CELL_FREE or VK_CELL_OCCUPIED
  Buffer<float> distance;             // metres to the nearest site cell
  Buffer<int> squared_cells;          // with DistanceFieldOptions::squared
};

// Not upstream: how Volume::CastRays reads its rays, how far it marches and what it samples at a hit (vk_cast_params)
struct CastOptions
{
  bool voxel_units = false;     // the origins, t_min, t_max and the returned t are in voxels, not metres
  bool distance_only = false;   // the colour fields of a hit's sample stay 0 and no colour is read
  float t_min = 0.0f;           // the stretch of each ray that is searched, along its normalised direction
  float t_max = 5.0f;
  int max_steps = 500;          // 1 .. 65536: a ray that needs more ends as VK_RAY_STEPS
};

// Not upstream: a ray of Volume::CastRays, in the layout vk_volume_cast_rays reads
struct Ray
{
  Vector3f origin;
  Vector3f direction;           // any length; a zero or non-finite direction is VK_RAY_INVALID
};

// Not upstream: how Volume::IntegrateRays reads its rays and ranges and what it fuses (vk_integrate_rays_params)
struct IntegrateRaysOptions
{
  bool voxel_units = false;           // the origins, the ranges, r_min and r_max are in voxels, not metres
  bool one_observation = false;       // a voxel's mean counts as one observation, not as one per ray through it
  float r_min = 0.1f;                 // a ray whose range lies outside [r_min, r_max] (a NaN included) carries no
  float r_max = 5.0f;                 //   measurement and is skipped: CastRays' t == 0 feeds in unchanged
  float max_distance_weight = 16.0f;  // the cap an integrator would apply (integrator.cu:7-13)
  int max_rounds = 8;                 // allocation rounds; 0: only blocks that exist are updated
};

// Volume::IntegrateRays (vk_volume_integrate_rays' eight counts)
struct IntegrateRaysCounts
{
  int integrated;       // valid rays with a measurement
  int unmeasured;       // valid rays without one
  int invalid;          // rays CastRays would call VK_RAY_INVALID
  int allocated;        // blocks this volume did not have before
  int rounds;           // allocation rounds that posted a request
  int blocks;           // blocks that took an update
  int voxels;           // voxels updated
  int lost;             // cell visits lost to a block that found no room
};

// Not upstream: how Volume::CarveRays reads its rays and ranges and what it carves (vk_carve_rays_params)
struct CarveRaysOptions
{
  bool voxel_units = false;           // the origins, the ranges, r_min, r_max and t_from are in voxels, not metres
  bool one_observation = false;       // a voxel's carves count as one observation, not as one per ray through it
  float r_min = 0.1f;                 // IntegrateRays' rule: a ray whose range lies outside [r_min, r_max] carries no
  float r_max = 5.0f;                 //   measurement and carves nothing
  float t_from = 0.0f;                // the carve starts here along the ray
  float max_distance_weight = 16.0f;  // the cap an integrator would apply (integrator.cu:7-13)
  int max_blocks = 1024;              // blocks a ray's carve may cross; what it does not reach is not carved
};

// Volume::CarveRays (vk_volume_carve_rays' eight counts)
struct CarveRaysCounts
{
  int carved;           // rays that carved
  int nothing;          // measured rays with nothing to carve: the carve would start at the band, or behind it
  int unmeasured;       // valid rays without a measurement
  int invalid;          // rays CastRays would call VK_RAY_INVALID
  int cut_short;        // rays whose carve ended at max_blocks
  int blocks;           // blocks that took an update
  int voxels;           // voxels updated
  unsigned carves;      // cells carved, over all rays
};

// Not upstream: how Volume::ColorRays reads its rays, ranges and colours and what it colours (vk_color_rays_params)
struct ColorRaysOptions
{
  bool voxel_units = false;           // the origins, the ranges, r_min, r_max and band are in voxels, not metres
  bool one_observation = false;       // a voxel's mean colour counts as one observation, not as one per ray through it
  float r_min = 0.1f;                 // IntegrateRays' rule: a ray whose range lies outside [r_min, r_max] carries no
  float r_max = 5.0f;                 //   measurement and colours nothing
  float band = 0.0f;                  // half width of the coloured stretch around the measurement; 0: the truncation length
  float max_color_weight = 16.0f;     // the cap a ColorIntegrator would apply (color_integrator.cu:125-129)
};

// Volume::ColorRays (vk_volume_color_rays' eight counts)
struct ColorRaysCounts
{
  int coloured;         // rays that coloured
  int colourless;       // measured rays without a colour: a channel outside [0, 1], a NaN included
  int unmeasured;       // valid rays without a measurement
  int invalid;          // rays CastRays would call VK_RAY_INVALID
  int blocks;           // blocks that took an update
  int voxels;           // voxels updated
  int not_near;         // voxels visited whose stored distance is not near a surface: left alone
  unsigned lost;        // cell visits lost to a block that does not exist
};

// Not upstream: how Volume::RegisterRays reads its rays and ranges and which returns take part (vk_register_rays_params)
struct RegisterRaysOptions
{
  bool voxel_units = false;           // the origins, the ranges, r_min and r_max are in voxels, not metres
  int iterations = 20;                // 1 .. 64 Gauss-Newton steps at most, enqueued at once
  float r_min = 0.1f;                 // IntegrateRays' rule: a ray whose range lies outside [r_min, r_max] carries no
  float r_max = 5.0f;                 //   measurement and takes no part
  float max_abs_distance = 0.75f;     // the band, in truncation lengths: a return that samples a distance this far from the
                                      //   mapped surface (a moved object, a spurious return) takes no part; the only outlier rule
};

// Not upstream: how Volume::ScorePoses and Volume::LocalizeRays read their rays and ranges and which returns count
// (vk_score_poses_params)
struct ScorePosesOptions
{
  bool voxel_units = false;           // the origins, the ranges, r_min and r_max are in voxels, not metres
  float r_min = 0.1f;                 // IntegrateRays' rule: a ray whose range lies outside [r_min, r_max] carries no
  float r_max = 5.0f;                 //   measurement and takes no part
  float max_abs_distance = 0.75f;     // the band, in truncation lengths: RegisterRays' residual test
};

// Volume::ScorePoses: how well one candidate pose explains a sweep (vk_pose_score)
struct PoseScore
{
  int measured;           // valid rays with a measurement
  int sampled;            // of those, endpoints where the map holds all eight voxels
  int residuals;          // of those, |D| below the band: what RegisterRays would compare at this pose
  int invalid;            // invalid rays
  long long sum_abs;      // sum of rint(|D| * 2^20) over the residuals: integers, so the order of the rays does not matter
  long long sum_squares;  // sum of rint(D * D * 2^20)
  double MeanAbs() const { return residuals > 0 ? double(sum_abs) / 1048576.0 / residuals : 0.0; }      // truncation lengths
  double Rms() const { return residuals > 0 ? std::sqrt(double(sum_squares) / 1048576.0 / residuals) : 0.0; }
};

// Volume::LocalizeRays: RegisterRays' result and the candidate it started from
struct Localization : Registration
{
  int best_index;         // -1: no candidate reached min_residuals; nothing was refined and `pose` is the identity
};

class Block;
struct Frame;
class HashEntry;
class Voxel;

class Volume
{
  public:
    Volume(int main_block_count, int excess_block_count);
    virtual ~Volume();

    // ---- geometry ----
    int GetMainBlockCount() const;
    int GetExcessBlockCount() const;
    float GetVoxelLength() const;
    void SetVoxelLength(float length);
    float GetTruncationLength() const;
    void SetTruncationLength(float length);
    const Vector2f& GetDepthRange() const;
    void SetDepthRange(const Vector2f& range);
    void SetDepthRange(float min, float max);

    // ---- per frame: allocate what the depth image touches, list what is visible ----
    void SetView(const Frame& frame);
    // `rounds` consecutive SetView(frame) calls (the app makes three per frame, vulcan.cu:316-318)
    // in one: the later rounds run on the device, and only when the round before lost a request
    void SetView(const Frame& frame, int rounds);
    // frame.ComputeNormals(); SetView(frame, rounds); in one call (not upstream): with a LightIntegrator
    // attached the normals are computed inside SetView's request pass (vk_light_prep.normals_out)
    void ComputeNormalsAndSetView(Frame& frame, int rounds = 1);

    // ---- storage ----
    const Buffer<HashEntry>& GetHashEntries() const;
    const Buffer<int>& GetAllocatedBlocks() const;
    const Buffer<int>& GetVisibleBlocks() const;   // first call after SetView syncs
    const Buffer<Voxel>& GetVoxels() const;
    Buffer<Voxel>& GetVoxels();

    vk_volume ToVk() const;                        // device view for the C ABI
    void GetCounters(int32_t* counters) const;     // blocking readback of the VK_CTR_PUBLIC counters
    // Not upstream: blocks of the pool in use, min(capacity, capacity - 1 - free-slot pointer) (blocking readback). The
    // pointer itself keeps falling once the pool is empty (upstream's does too, src/volume.cu:352-356): VK_CTR_DROPPED
    // counts the requests that found it empty.
    int GetAllocatedBlockCount() const;
    // Not upstream (round 6): SetView(frame, rounds) at a pose that is still ON THE DEVICE — the vk_transform a tracker's
    // launches in front of this call leave there — so that a tracking loop can enqueue SetView behind its Track before it waits
    // for the pose (vk_volume_set_view_at_device_pose; PyramidTracker<DepthTracker>::ComputeNormalsTrackAndSetView uses it).
    // frame.depth_to_world_transform is ignored. false: not possible in this state (a frame announced by Tracer::Trace, a
    // request stream, the three-launch test form) — nothing was launched, the caller calls SetView once it has the pose.
    bool SetViewAtDevicePose(const Frame& frame, const vk_transform* pose_device, int rounds = 1);

    // Not upstream (src/volume.cu:304-368 never returns a slot): give the blocks `rule` names back to the pool, compact
    // the hash table and rebuild the free list (vk_volume_release_blocks) — also the way back from an exhausted pool,
    // whose leaked slots and never-written excess entries it recovers even with an empty rule. Between SetView calls
    // only: throws while a frame announced by Tracer::Trace(keyframe, next_frame) is outstanding. The visible list is
    // empty afterwards (the next SetView rebuilds it); the raycast bounds and the light preparation made ahead are void.
    // One blocking readback (the four counts).
    ReleaseCounts ReleaseBlocks(const ReleaseRule& rule);

    // Not upstream (its Volume is a process-wide singleton, src/volume.cu:17-21): fuse `other` — same voxel and truncation
    // length, on this device, any bucket and pool size — into this volume (vk_volume_merge). The blocks this volume lacks
    // are allocated, then every voxel's running average goes on with the other voxel's value and weight; every block of
    // `other` is fused once, in as many calls of the entry point as its allocation rounds take. `other` is only read.
    // Between SetView calls only: throws while either volume has a frame announced by Tracer::Trace(keyframe, next_frame).
    // The visible list is empty afterwards (the next SetView rebuilds it); the raycast bounds and the light preparation
    // made ahead are void. Blocking readbacks (the six counts, VK_CTR_DROPPED).
    MergeCounts Merge(const Volume& other, const MergeOptions& options = MergeOptions());
    // ... with the blocks of a pack in the other volume's place (vk_volume_merge_packed): for a pack made without options
    // from a volume, the state and the counts Merge(that volume) leaves. The pack's voxel and truncation length must be
    // this volume's. A pack without blocks: no call. Otherwise as Merge(other).
    MergeCounts Merge(const PackedVolume& pack, const MergeOptions& options = MergeOptions());
    // Not upstream: this volume's blocks as a PackedVolume (vk_volume_pack) — a call that counts, one blocking read of the
    // count, an allocation of exactly that size, the call that packs. The volume is only read: like Sample it is allowed
    // while a frame announced by Tracer::Trace(keyframe, next_frame) is outstanding.
    PackedVolume Pack(const PackOptions& options = PackOptions()) const;
    // Not upstream: a map file (PackedVolume::Save) as a fresh volume of the given table sizes, which need not be those
    // of the volume that was saved: the file's voxel and truncation length, and Merge(pack) with both caps 32767, which
    // into empty blocks is a copy. Throws when the blocks do not fit.
    static std::shared_ptr<Volume> Load(const std::string& path, int main_block_count, int excess_block_count);
    // ... through the rigid pose Tdst_src (x in this volume's frame = Tdst_src * x in `other`'s, metres): the two need not
    // share a world frame or a voxel lattice (vk_volume_merge_posed). Every voxel of the blocks of this volume that `other`'s
    // blocks reach takes a trilinear sample of `other` at its own centre carried back; a reached block no sample falls into
    // stays allocated and empty (ReleaseBlocks with `unobserved` gives those back). Otherwise as Merge(other).
    MergePoseCounts Merge(const Volume& other, const Transform& Tdst_src, const MergeOptions& options = MergeOptions());
    // ... when `other` has another voxel length (up to a factor of 4 either way), another truncation length, or both
    // (vk_volume_merge_resampled). Every voxel takes the mean of supersample^3 (1 .. 4 per axis) trilinear samples of
    // `other` spread over the voxel — a box filter, so a coarser copy does not alias; 0: as many per axis as voxels of
    // `other` lie along one of this volume's — and a stored distance is carried from `other`'s truncation length into this
    // volume's: beyond this volume's band it saturates at 1 or, behind the surface, is left out. At equal lengths with
    // supersample 1 this is Merge(other, Tdst_src), byte for byte. Otherwise as Merge(other, Tdst_src).
    MergePoseCounts MergeResampled(const Volume& other, const Transform& Tdst_src, int supersample = 0,
        const MergeOptions& options = MergeOptions());
    // Not upstream: refine that pose from the two volumes themselves (vk_volume_register) — Gauss-Newton on the TSDFs,
    // every voxel of `other` within `max_abs_distance` truncation lengths of the surface against the trilinear sample of
    // this volume where `start` (then the refined pose) carries it. `start` has to bring the two surfaces within roughly
    // a truncation length of each other where they overlap: the call refines a guess, it does not search. Both volumes
    // are only read; at most `iterations` steps (1 .. 64), enqueued at once; blocking readbacks at the end.
    Registration Register(const Volume& other, const Transform& start, int iterations = 20, float max_abs_distance = 0.75f);

    // Not upstream: the volume's field at `count` arbitrary points (vk_volume_sample) — per point the trilinear sample of
    // the stored voxels as a Voxel, the way Merge(other, pose) samples at a voxel's centre, and the gradient of the
    // distance (x, y, z in truncation lengths per voxel, then 1 where it exists, else four zeros). The points are in
    // metres in the frame that `pose` (null: the volume's own) carries into the volume's. A field without a sample is
    // Voxel::Empty()'s: distance 1, weight 0. All three buffers are device memory; one of samples_dev / gradients_dev may
    // be null (gradients_dev is 16-byte aligned). The volume is only read: one launch on Device::GetStream(), nothing is
    // read back.
    void Sample(const Vector3f* points_dev, int count, Voxel* samples_dev, Vector4f* gradients_dev, const Transform* pose = nullptr,
        const SampleOptions& options = SampleOptions()) const;

    // Not upstream: how far every cell of a dense grid is from the nearest surface (vk_volume_distance_field) — the
    // clearance a planner asks for, which the stored distance cannot give beyond one truncation length. The grid is
    // classified (unknown, free, occupied: ClassifyCells alone does that much) and every cell takes the exact Euclidean
    // distance, centre to centre and in metres, to the nearest cell whose class is in options.site_mask; +infinity where
    // none lies within options.max_cells. Blocks exist only inside the truncation band, so open space in front of it reads
    // unknown. The volume is only read — like Sample both are allowed while a frame is announced — in one enqueue on
    // Device::GetStream(); nothing is read back.
    void DistanceField(const CellGrid& grid, const DistanceFieldOptions& options, DistanceFieldBuffers& buffers) const;
    void ClassifyCells(const CellGrid& grid, float occupied_below, Buffer<unsigned char>& classes) const;

    // Not upstream: what each of `count` arbitrary rays hits first in the volume (vk_volume_cast_rays) — the raycast's
    // march along rays that are no pixels of a camera: a line of sight, a simulated range sensor, picking. Per ray the
    // outcome (VK_RAY_MISS, _HIT, _STEPS, _INVALID) in status_dev, the distance along the normalised direction in t_dev
    // (0 without a hit) and, where asked for, Sample's voxel and gradient at the hit (Voxel::Empty() and four zeros
    // without one). A surface is reported only where the ray crosses it from its observed free side. The rays are in the
    // frame that `pose` (null: the volume's own) carries into the volume's. All buffers are device memory; samples_dev
    // and gradients_dev may be null (gradients_dev is 16-byte aligned). The volume is only read: one launch on
    // Device::GetStream(), nothing is read back.
    void CastRays(const Ray* rays_dev, int count, float* t_dev, int* status_dev, Voxel* samples_dev = nullptr,
        Vector4f* gradients_dev = nullptr, const Transform* pose = nullptr, const CastOptions& options = CastOptions()) const;

    // Not upstream: fuse `count` range measurements along arbitrary rays (vk_volume_integrate_rays) — a LiDAR sweep, a
    // fisheye depth camera, a point cloud seen from known origins, or what CastRays returned for another volume.
    // ranges_dev[i] is the distance along the normalised direction of rays_dev[i], both in the frame that `pose` (null:
    // the volume's own) carries into the volume's. The blocks within one truncation length either side of a measurement
    // are allocated, then every voxel whose cell a ray crosses inside that band continues its running average with the
    // mean of what the rays through it measured; colours are left alone, and the order of the rays does not matter.
    // Between SetView calls only: throws while a frame announced by Tracer::Trace(keyframe, next_frame) is outstanding.
    // The visible list is empty afterwards (the next SetView rebuilds it); the raycast bounds and the light preparation
    // made ahead are void. Both buffers are device memory and only read. Blocking readbacks (the eight counts,
    // VK_CTR_DROPPED); count == 0 does nothing.
    IntegrateRaysCounts IntegrateRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform* pose = nullptr,
        const IntegrateRaysOptions& options = IntegrateRaysOptions());

    // Not upstream: carve the free space in front of `count` range measurements (vk_volume_carve_rays) — what is no
    // longer there. Rays, ranges and pose are IntegrateRays'. Every voxel of an existing block whose cell a measured ray
    // crosses between options.t_from and the start of the band IntegrateRays fuses takes an observation of the distance 1,
    // "free"; colours are left alone, and the order of the rays does not matter. Nothing is allocated: absent blocks are
    // passed over, and the hash table, the free list, the visible list and what was made ahead stay as they are. Between
    // SetView calls only: throws while a frame announced by Tracer::Trace(keyframe, next_frame) is outstanding. Both
    // buffers are device memory and only read. One blocking readback (the eight counts); count == 0 does nothing.
    CarveRaysCounts CarveRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform* pose = nullptr,
        const CarveRaysOptions& options = CarveRaysOptions());

    // Not upstream: fuse a colour per range ray (vk_volume_color_rays) — a LiDAR return coloured by a camera, or the colour
    // CastRays returned for another volume. Rays, ranges and pose are IntegrateRays'; colors_dev[i] is r, g, b in [0, 1].
    // Every voxel of an existing block whose cell a coloured ray crosses within options.band of its measurement, and whose
    // stored distance is near the surface, continues its colour's running average with the mean colour of the rays
    // through it; the order of the rays does not matter. Nothing is allocated — a cell without a block is a lost visit:
    // call IntegrateRays first — and the distances, the hash table, the free list, the visible list and what was made
    // ahead stay as they are. At most 1 << 21 rays a call. Between SetView calls only: throws while a frame announced by
    // Tracer::Trace(keyframe, next_frame) is outstanding. The three buffers are device memory and only read. One blocking
    // readback (the eight counts); count == 0 does nothing.
    ColorRaysCounts ColorRays(const Ray* rays_dev, const float* ranges_dev, const Vector3f* colors_dev, int count,
        const Transform* pose = nullptr, const ColorRaysOptions& options = ColorRaysOptions());

    // Not upstream: where the sensor is (vk_volume_register_rays) — refine the pose Tvolume_rays of a sweep of `count` range
    // rays, the pose IntegrateRays, CarveRays and ColorRays take as given, by Gauss-Newton on "the endpoint of a return lies
    // on the mapped surface": every measured ray's endpoint is carried into the volume through `start` (then the refined
    // pose) and the trilinear sample there is driven to 0. Rays and ranges are IntegrateRays'. `start` has to bring the
    // endpoints within roughly a truncation length of the surface: the call refines a guess, it does not search, and a
    // sweep that sees a single plane does not fix the pose (the step is then zero and the call reports convergence where
    // it started). The volume is only read and the call writes nothing of it: like Sample and CastRays it is allowed while
    // a frame announced by Tracer::Trace(keyframe, next_frame) is outstanding. Both buffers are device memory and only
    // read. All steps are enqueued at once on Device::GetStream(); blocking readbacks at the end; count == 0 does nothing.
    Registration RegisterRays(const Ray* rays_dev, const float* ranges_dev, int count, const Transform& start,
        const RegisterRaysOptions& options = RegisterRaysOptions()) const;

    // Not upstream: how well each of many candidate poses Tvolume_rays explains a sweep (vk_volume_score_poses) — the search
    // RegisterRays does not make: a sensor switched on somewhere in a known map, a tracker that lost its pose, a loop closure
    // to verify. Every ray is put to RegisterRays' residual test at every pose; producing the candidates is the caller's.
    // At most 65 536 poses, 1 << 22 rays and 1 << 28 pairs a call. The volume is only read: allowed while a frame is
    // announced. One blocking readback (the scores); count == 0 does nothing and gives scores of zeros.
    std::vector<PoseScore> ScorePoses(const Ray* rays_dev, const float* ranges_dev, int count, const std::vector<Transform>& poses,
        const ScorePosesOptions& options = ScorePosesOptions()) const;

    // Not upstream: where the sensor is, from far away — ScorePoses at `poses`, the best of them chosen on the device (the
    // most residuals, then the smallest sum of |D|, then the smallest index: vk_volume_score_poses_best) and RegisterRays
    // from it, all enqueued before anything is read. A best candidate with fewer than `min_residuals` (>= 1) residuals is
    // none: best_index is -1 and nothing is refined. Rays, ranges and options are RegisterRays'. Allowed while a frame is
    // announced; count == 0 does nothing (best_index -1).
    Localization LocalizeRays(const Ray* rays_dev, const float* ranges_dev, int count, const std::vector<Transform>& poses,
        int min_residuals, const RegisterRaysOptions& options = RegisterRaysOptions()) const;

    // Raycast bounds prepared ahead of time (vk_view_bounds, not upstream): a Tracer
    // registers its scratch buffer and settings here, the integrators then compute
    // the bounds of the view they integrate inside their own launch and
    // Tracer::Trace skips that pass when it raycasts the same view. SetView (a new
    // visible list) invalidates the record. nullptr while no Tracer is attached.
    vk_view_bounds* GetViewBounds() const;
    void AttachViewBounds(float* scratch, int bounds_width, int bounds_height, const Vector2f& depth_range) const;
    void DetachViewBounds(const float* scratch) const;   // no-op unless `scratch` is the attached one

    // LightIntegrator's per-pixel preparation, ahead of time (vk_light_prep, not upstream): a
    // LightIntegrator registers its mask / record buffers here and SetView fills them in its own
    // request pass, for the Integrate of the same frame that follows (the frame must not be
    // modified in between). nullptr while nothing is attached.
    vk_light_prep* GetLightPreparation() const;
    void AttachLightPreparation(float* mask, float* records, int capacity_pixels, float depth_threshold) const;
    void DetachLightPreparation(const float* mask) const;   // no-op unless `mask` is the attached one

    // Not upstream (which runs everything on stream 0): SetView's request pass on a stream of its own
    // (vk_volume_set_view_rounds_split), so that it runs beside the PREVIOUS frame's Tracer::Trace instead of behind it. For
    // callers that know a frame's pose before the previous frame's raycast has finished — fusion at given poses; a tracking
    // loop gains nothing, its pose comes out of that raycast. The request pass then waits only for the previous Integrate
    // (the integrators call NoteIntegrated): whatever it reads — the frame's depth image, and colour / normal images when a
    // LightIntegrator's preparation rides along — must be complete without work enqueued on Device::GetStream() after that
    // Integrate (ComputeNormalsAndSetView computes the normals inside the pass; FrameUploader::Acquire takes the stream to wait on).
    void EnableRequestStream();
    void* GetRequestStream() const { return request_stream_; }
    void NoteIntegrated() const;

    // Not upstream: the record of a request pass made AHEAD of its SetView (vk_requests_ahead) — by
    // Tracer::Trace(keyframe, next_frame), inside the raycast's own launch. SetView(next_frame) then launches only its
    // handle + visibility pass; any other SetView while the record is valid throws (the announced frame's requests
    // are in the volume and have to be handled first).
    vk_requests_ahead* GetRequestsAhead() const { return &requests_ahead_; }
    // The way out of an announced frame that will not be fused as announced (vk_requests_ahead_cancel): its SetView is
    // completed from the record — `rounds` as in SetView — and any frame may follow. No-op without a valid record.
    void CancelRequestsAhead(int rounds = 1);

  protected:
    // the four stages of SetView, in call order
    void ResetBlockVisibility();
    void CreateAllocationRequests(const Frame& frame);
    void HandleAllocationRequests();
    void UpdateBlockVisibility(const Frame& frame);

    int GetBufferSize() const;
    void ResetBufferSize() const;

    Buffer<Voxel> voxels_;
    Buffer<HashEntry> hash_entries_;
    Buffer<int> free_voxel_blocks_;
    Buffer<AllocationType> allocation_types_;
    Buffer<Block> allocation_blocks_;
    Buffer<Visibility> block_visibility_;
    mutable Buffer<int> visible_blocks_;
    Buffer<int> counters_;
    Buffer<unsigned char> release_workspace_;   // ReleaseBlocks: allocated by the first call
    Buffer<int> release_counts_;
    Buffer<unsigned char> merge_workspace_;     // Merge: allocated by the first call, again for a source of another size
    Buffer<int> merge_counts_;
    Buffer<unsigned char> merge_packed_workspace_;   // Merge of a pack: again for a pack of another size
    Buffer<int> merge_packed_counts_;
    mutable Buffer<unsigned char> pack_workspace_;   // Pack: allocated by the first call
    mutable Buffer<int> pack_counts_;
    Buffer<unsigned char> merge_pose_workspace_;   // Merge through a pose: again for another pair of sizes
    Buffer<int> merge_pose_counts_;
    Buffer<unsigned char> merge_resample_workspace_;   // MergeResampled: again for another pair of sizes or another ratio
    Buffer<int> merge_resample_counts_;
    // a registration's device buffers, and what is done with them before and after the loop
    struct RegistrationBuffers
    {
      Buffer<float> floats;                        // the pose (32), the system (48), the update (6)
      Buffer<int> ints;                            // the state (2), the counts (4)
      vk_transform* pose = nullptr;
      float* system = nullptr;
      float* update = nullptr;
      int* state = nullptr;
      int* counts = nullptr;
      void Begin(const Transform* seed);           // allocated by the first call; a seed is uploaded and the state zeroed
      Registration Read() const;                   // one blocking read of each buffer
    };
    Buffer<unsigned char> register_workspace_;     // Register: again for a source of another size
    RegistrationBuffers register_;
    mutable Buffer<float> sample_pose_;            // Sample, CastRays, IntegrateRays, CarveRays, ColorRays: the pose on the device (32)
    mutable Buffer<unsigned char> field_workspace_;   // DistanceField: again for a grid of another size
    Buffer<unsigned char> rays_workspace_;         // IntegrateRays: allocated by the first call
    Buffer<int> rays_counts_;
    Buffer<unsigned char> carve_workspace_;        // CarveRays: allocated by the first call
    Buffer<int> carve_counts_;
    Buffer<unsigned char> color_rays_workspace_;   // ColorRays: allocated by the first call
    Buffer<int> color_rays_counts_;
    mutable Buffer<unsigned char> register_rays_workspace_;   // RegisterRays: again for another number of rays
    mutable RegistrationBuffers register_rays_;               // RegisterRays and LocalizeRays
    mutable Buffer<unsigned char> score_poses_workspace_;     // ScorePoses: again for another number of rays or poses
    mutable Buffer<unsigned char> score_poses_scores_;        // [poses] vk_pose_score
    mutable Buffer<float> score_poses_poses_;                 // [poses] vk_transform
    mutable Buffer<int> score_poses_best_;                    // LocalizeRays: the chosen index (1)

    Vector2f depth_range_;
    int max_block_count_;
    int main_block_count_;
    int excess_block_count_;
    float truncation_length_;
    float voxel_length_;
    bool empty_;
    mutable bool visible_count_stale_;
    mutable vk_view_bounds view_bounds_;
    mutable vk_light_prep light_prep_;
    mutable vk_requests_ahead requests_ahead_;
    void* request_stream_;              // EnableRequestStream(): nullptr = everything on Device::GetStream()
    void* requested_;                   // event behind the request pass
    void* integrated_;                  // event behind the last Integrate
    mutable bool integrated_recorded_;
    mutable bool pool_exhaustion_noted_ = false;
    void NotePoolExhaustion(int32_t dropped) const;
    mutable int32_t* normals_late_;     // pinned: vk_view_bounds.late_host of the attached tracer's record
    // a call's workspace of `bytes` (again for another size; 0: no call follows) and its `count` counts, allocated by the first
    static void Sized(Buffer<unsigned char>& workspace, size_t bytes, Buffer<int>& counts, size_t count = 8);

  private:
    // what the volume operations above share on the caller's side
    void AssertNoFrameAnnounced() const;                               // between SetView calls only
    const vk_transform* PoseOnDevice(const Transform* pose) const;     // uploaded into sample_pose_; null stays null
    static int RayFlags(bool voxel_units, bool one_observation = false);           // VK_RAYS_*
    static std::array<int32_t, 8> EightCounts(const Buffer<int>& counts_dev);      // one blocking read
    int ScorePosesBuffers(int count, const std::vector<Transform>& poses) const;    // the candidates uploaded: how many
    void VoidMadeAhead() const;                 // the raycast bounds and the light preparation made for the old table
    void EmptyVisibleList() const;              // VK_CTR_VISIBLE is 0 until the next SetView
    // the Merge overloads: `call(dst, src, counts_dev, workspace)` is the library call with `merge` among its parameters,
    // made again with VK_MERGE_CONTINUE until every block had its turn; `total` takes the `count` (6 or 8) summed counts.
    // `other` null: the source is a pack, and `src` of the call is null
    template <typename Call>
    void MergeRounds(const Volume* other, vk_merge_params& merge, Buffer<unsigned char>& workspace, size_t bytes,
        Buffer<int>& counts_dev, int count, int32_t* total, Call call);
    void Initialize();
    Volume(const Volume&);              // not copyable
    Volume& operator=(const Volume&);
};

} // namespace vulcan
