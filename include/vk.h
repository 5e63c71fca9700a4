/*
 * vk.h — C ABI of the MI355X-native fusion + raycast hot path (libvk_hip.so).
 *
 * This is the drop-in boundary. The reference (mkaspr/Vulcan) has no FFI: its
 * boundary is the C++ class surface Volume / Integrator(+3) / Tracer / Frame /
 * DepthTracker plus the free-function layer tracer.cuh:14-32 / frame.cuh.  Each
 * entry point below replaces the body of one of those methods (cited as
 * `ref: file:line`, paths relative to the reference tree); the C++ classes in
 * vulcan_amd/host/ keep the reference's names and forward here.
 *
 * Conventions
 *  - plain C: PODs, raw DEVICE pointers, ints, floats. No C++/torch types.
 *  - every function returns 0 on success, a hipError_t value (>0) on a HIP
 *    failure, or a negative VK_ERR_* code on bad arguments. Nothing throws.
 *    vk_error_string() maps a code to text.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream). All
 *    work is stream-ordered and asynchronous unless the function name ends in
 *    `_sync` or the comment says "blocking".
 *  - matrices are 4x4 column-major float[16], exactly the reference's
 *    Matrix4f (matrix.h:320-333); vk_transform carries matrix + cached inverse
 *    like Transform (transform.h:168-170). The inverse is never recomputed.
 *  - counts that the reference reads back to the host between kernels
 *    (visible-block count volume.cu:494, patch count tracer.cpp:67) stay in
 *    device memory (vk_volume.counters); consumers read them on the device.
 */
#ifndef VK_H_
#define VK_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_API __attribute__((visibility("default")))

/* ---------------------------------------------------------------- PODs -- */

/* ref: include/vulcan/voxel.h:43-49 — 20 bytes, align 4 */
typedef struct vk_voxel {
  float   distance;
  float   color[3];
  int16_t distance_weight;
  int16_t color_weight;
} vk_voxel;

/* ref: include/vulcan/block.h:81-85 — 8 bytes. `pad` is uninitialised in the
 * reference; here it is always written as 0 in hash entries. */
typedef struct vk_block {
  int16_t origin[3];
  int16_t pad;
} vk_block;

/* ref: include/vulcan/hash.h:51-55 — 16 bytes */
typedef struct vk_hash_entry {
  vk_block block;
  int32_t  data;  /* voxel pool slot, -1 = unallocated */
  int32_t  next;  /* entry index of next in chain, -1 = end */
} vk_hash_entry;

/* ref: include/vulcan/tracer.h:13-22 — 16 bytes */
typedef struct vk_patch {
  int16_t origin[2];
  int16_t size[2];
  float   bounds[2];
} vk_patch;

/* ref: include/vulcan/projection.h:111-113 — focal length then centre */
typedef struct vk_projection {
  float fx, fy, cx, cy;
} vk_projection;

/* ref: include/vulcan/transform.h:168-170 */
typedef struct vk_transform {
  float m[16];    /* matrix_, column-major */
  float inv[16];  /* inv_matrix_ */
} vk_transform;

/* ref: include/vulcan/light.h:62-66 */
typedef struct vk_light {
  float intensity;
  float position[3];
} vk_light;

/* ref: include/vulcan/types.h:6-18 */
enum { VK_VISIBILITY_UNKNOWN = 0, VK_VISIBILITY_FALSE = 1, VK_VISIBILITY_TRUE = 2 };
enum { VK_ALLOC_NONE = 0, VK_ALLOC_MAIN = 1, VK_ALLOC_EXCESS = 2 };

enum {
  VK_BLOCK_RESOLUTION = 8,    /* block.h:13 */
  VK_BLOCK_VOXELS     = 512,  /* block.h:15 */
  VK_PATCH_MAX_SIZE   = 16    /* tracer.h:15 */
};

/* Per-volume device counters. The reference keeps these as file-scope
 * __device__ symbols shared by every Volume (volume.cu:17-21); here each
 * volume owns an int[VK_CTR_COUNT] in device memory, 8-byte aligned. */
enum {
  VK_CTR_VISIBLE    = 0,  /* buffer_size: number of entries in visible_blocks */
  VK_CTR_VOXEL_PTR  = 1,  /* voxel_pointer: top of the free-slot stack */
  VK_CTR_EXCESS_PTR = 2,  /* excess_pointer: next free excess entry */
  VK_CTR_PATCHES    = 3,  /* tracer patch count (tracer.h buffer_size_) */
  VK_CTR_REQUESTS   = 4,  /* requests seen by the last handle pass */
  VK_CTR_DROPPED    = 5,  /* requests dropped so far: pool or excess list exhausted */
  VK_CTR_PENDING_ALL    = 6,  /* internal: pointer updates of a handle pass, not yet folded in */
  VK_CTR_PENDING_EXCESS = 7,
  VK_CTR_ROUNDS     = 8,  /* SetView rounds run so far by vk_volume_set_view* (cumulative) */
  VK_CTR_UNSETTLED  = 9,  /* the last vk_volume_set_view* left a request unanswered: lost to a bucket
                             contest in its last round, or dropped (pool / excess list exhausted), or
                             more losers than the retry list holds — another SetView call has work */
  VK_CTR_CONTENDED  = 10, /* internal: the request pass lost a request to a bucket contest */
  VK_CTR_TICKET     = 11, /* internal: handle workgroups that have finished the first round */
  VK_CTR_RETRY_COUNT = 12, /* internal [2]: keys filed in the two retry lists */
  VK_CTR_RETRY_OVERFLOW = 14, /* internal: a retry list (or the ordering buffer of a later round) was too small */
  VK_CTR_DROPPED_NOW = 15, /* internal: the current call dropped a request */
  VK_CTR_ORIGIN_SEEN = 16, /* internal: a ray met block (0,0,0) while the main entry of its bucket was
                              unallocated — such an entry compares equal to that block (volume.cu:186-191),
                              so the block counts as present until the entry is taken by another block */
  VK_CTR_POSTED     = 17, /* internal: buckets that received their first request in the current request pass
                             (may exceed VK_POSTED_SLOTS: then the handle pass scans the request flags instead) */
  VK_CTR_ARRIVALS   = 18, /* internal [2], one 64-bit word: the arrivals of the workgroups of the handle + visibility
                             launch of vk_volume_set_view* (zero between calls) */
  VK_CTR_BANDED     = 20, /* internal: the banded visible lists (below) hold exactly VK_CTR_VISIBLE entries — set to that
                             count by the handle + visibility launch of vk_volume_set_view* when it has listed every
                             visible entry in them, to -1 by everything else that writes the visible list */
  VK_CTR_PUBLIC     = 24, /* what vk_volume_read_counters_sync copies */
  /* behind the counters, for vk_volume_set_view_rounds: the blocks whose request lost its bucket in
   * the round before — two open-addressing sets of VK_RETRY_SLOTS 64-bit request keys (current
   * round / next round) and, for each, the list of the slots in use (VK_RETRY_KEYS ints) */
  VK_RETRY_SLOTS    = 65536,
  VK_RETRY_KEYS     = 8192,
  /* then the buckets with a request of the current request pass, in order of arrival (bit 31: an
   * EXCESS request), and for each the last entry of its chain: what the handle pass of
   * vk_volume_set_view* works from when there are few */
  VK_POSTED_SLOTS   = 2048,
  /* then the visible entries once more, binned by the image row band of a depth pixel whose ray touched the block
   * (VK_BANDS bands of height / VK_BANDS rows): VK_BANDS counts, then VK_BANDS lists of VK_BAND_SLOTS entry indices.
   * The integrate kernels deal the bands to the XCDs, so that each XCD's L2 holds the image rows its blocks project
   * to (round 4). A band with more entries than slots makes the integrate kernels use the plain list. */
  VK_BANDS          = 8,
  VK_BAND_SLOTS     = 16384,
  VK_CTR_COUNT      = 24 + 2 * 2 * 65536 + 2 * 8192 + 2 * 2048 + 8 + 8 * 16384
};

enum {
  VK_OK              =  0,
  VK_ERR_ARGUMENT    = -1,  /* null pointer / non-positive size */
  VK_ERR_UNSUPPORTED = -2,
  VK_ERR_NO_DEVICE   = -3,
  VK_ERR_TIMEOUT     = -6   /* a bounded wait INSIDE a launch expired (vk_trace_normals_settle); what it says was not
                               written has been recomputed, or the call must be repeated. (-4, -5: vk_comm.h) */
};

/* Device-memory view of a Volume (ref: include/vulcan/volume.h:89-116).
 * The caller owns every buffer; the library never allocates or frees them. */
typedef struct vk_volume {
  vk_voxel*      voxels;             /* [max_block_count * 512]      voxels_            */
  vk_hash_entry* hash_entries;       /* [max_block_count]            hash_entries_      */
  int32_t*       free_voxel_blocks;  /* [max_block_count]            free_voxel_blocks_ */
  uint8_t*       allocation_types;   /* [main_block_count], 16-byte aligned             allocation_types_  */
  vk_block*      allocation_blocks;  /* [main_block_count], 8-byte aligned  allocation_blocks_ */
  uint8_t*       block_visibility;   /* [max_block_count], 4-byte aligned, the allocation padded to a multiple of
                                        4 bytes (the last bytes are accessed as part of their word)  block_visibility_  */
  int32_t*       visible_blocks;     /* [max_block_count]            visible_blocks_    */
  int32_t*       counters;           /* [VK_CTR_COUNT]               (volume.cu:17-21)  */
  int32_t        main_block_count;
  int32_t        excess_block_count;
  float          voxel_length;       /* volume.cu:376 default 0.008 */
  float          truncation_length;  /* volume.cu:375 default 0.04  */
  float          min_depth;          /* volume.cu:374 default 0.1   */
  float          max_depth;          /*               default 5.0   */
} vk_volume;

/* Depth / colour / normal images of a Frame (ref: include/vulcan/frame.h:11-32)
 * row-major, no pitch; colour and normals are packed 12-byte float3. */
typedef struct vk_frame {
  const float*  depth;        /* [height*width]   */
  const float*  color;        /* [color_height*color_width*3] or NULL */
  const float*  normals;      /* [height*width*3] or NULL */
  int32_t       width;        /* depth_image (and normal_image) size */
  int32_t       height;
  /* color_image size (frame.h:21-25 holds three independent images). 0 = same
   * as the depth image. ColorIntegrator::IntegrateColor bounds-tests and
   * strides with THIS size (color_integrator.cu:183-184); LightIntegrator
   * indexes colour with the depth image's size (light_integrator.cu:333-334,
   * "TODO: handle different depth and color images sizes" :179), which is an
   * out-of-bounds read when they differ: the light entry points return
   * VK_ERR_ARGUMENT for such a frame instead. */
  int32_t       color_width;
  int32_t       color_height;
  vk_projection depth_projection;
  vk_projection color_projection;
  vk_transform  depth_to_world;   /* Twd */
  vk_transform  depth_to_color;   /* Tcd */
  /* Identity of the images' CONTENT, maintained by the caller: a value that changes whenever
   * a pixel of the depth, colour or normal image changes (the class layer stamps its images on
   * every write it can see, image.h). 0 = unknown. Only vk_volume_set_view_prepare /
   * vk_light_prepared look at it: work done ahead for a frame is reused for the same
   * content only, never for "the same pointers". No reference counterpart. */
  uint64_t      content_id;
} vk_frame;

/* -------------------------------------------------------------- test aids -- */

/* Process-wide switches with which the test suites force paths that real input reaches rarely, and two
 * measurement options. Nothing on a call path reads the environment: a caller sets these once (any thread,
 * before the calls they concern); the library reads them with relaxed atomic loads. No reference counterpart. */
typedef struct vk_test_hooks {
  int32_t posted_capacity;    /* buckets the posted list of vk_volume_set_view* holds; < 0: VK_POSTED_SLOTS. A small
                                 list sends the handle pass to the request flags */
  int32_t retry_capacity;     /* distinct keys per retry list; <= 0: VK_RETRY_KEYS. A small list overflows on purpose */
  int32_t set_view_unfused;   /* 1: vk_volume_set_view* as three launches (requests, handle + later rounds,
                                 visibility) instead of two: the second implementation the tests compare with */
  int32_t force_loop_abort;   /* 1: every one-launch Gauss-Newton loop ends at once with VK_TRACK_ABORTED, as after the
                                 exchange timeout, so that the launch-per-stage fallback can be tested */
  int32_t loop_grid_cap;      /* > 0: at most this many workgroups per loop kernel (a device with fewer CUs) */
  int32_t loop_cooperative;   /* 1: loop kernels go through hipLaunchCooperativeKernel (the runtime then refuses a
                                 grid that cannot be resident; +4..6.5 us per Track) */
  int32_t force_normals_expiry; /* 1: the normals workgroups of the NEXT vk_trace_ahead_requests launch find their wait
                                 expired at once (a target no counter reaches, no polls) — then back to 0 by itself: the
                                 error path of vk_trace_normals_settle under test */
} vk_test_hooks;

VK_API int vk_test_hooks_set(const vk_test_hooks* hooks);   /* NULL: everything back to its default */
VK_API int vk_test_hooks_get(vk_test_hooks* out);

/* The library's count of one-launch Gauss-Newton loops (vk_icp_track & co.). Every such launch tags the words its
 * workgroups exchange with 22 bits of this count (1 + count mod (2^22 - 1)), so the tags repeat every 2^22 - 1 launches —
 * about ten minutes of tracking. The library keeps the repeat from ever being seen: a tracker's `workspace` is cleared
 * in front of a launch whenever it is new to the library, was last cleared 2^21 or more launches ago, or was written by
 * a launch-per-stage loop in between (vulcan_amd/csrc/vk_runtime.hip, vk_loop_epoch_begin). What the caller owes: nothing
 * but the library writes a workspace between two calls that use it, and a workspace made of memory that has been back at an
 * allocator since the library last saw that address is zeroed by the caller first (vk_memset) — the library knows areas by
 * their address and cannot see a free (the host layers zero a workspace when they allocate it). This entry point lets a test put the count right
 * in front of a repeat instead of tracking for ten minutes: `set_to` (may be NULL) replaces the count, `count_now` and
 * `clears` (may be NULL) receive the count and the number of clears enqueued so far. No reference counterpart (upstream's
 * loop, src/tracker.cpp:53-63, has no launch tags). */
VK_API int vk_test_hooks_loop_count(const uint64_t* set_to, uint64_t* count_now, uint64_t* clears);

/* ------------------------------------------------------ library / device -- */

VK_API const char* vk_error_string(int code);
VK_API int vk_version(void);                       /* 100*major + minor */

/* The binary interface has changed between rounds (struct fields, the size of the counters block — VK_CTR_COUNT ints,
 * of which vk_volume_read_counters_sync copies VK_CTR_PUBLIC = 24 —, the meaning of vk_frame.content_id), and a caller
 * built against an older vk.h would hand the library buffers that are too small. VK_ABI_VERSION counts those changes;
 * vk_abi_check compares what the CALLER was compiled against with what the LIBRARY was: call it once after loading
 *   vk_abi_check(VK_ABI_VERSION, sizeof(vk_volume), sizeof(vk_frame), VK_CTR_COUNT)
 * and refuse to go on unless it returns VK_OK (VK_ERR_UNSUPPORTED otherwise). The class layer (vulcan_amd/host) and the
 * Python binding do. New struct fields are appended; a change of VK_CTR_COUNT bumps the version. No reference counterpart. */
#define VK_ABI_VERSION 7
VK_API int vk_abi_version(void);
VK_API int vk_abi_check(int header_abi_version, size_t sizeof_vk_volume, size_t sizeof_vk_frame, int ctr_count);
VK_API int vk_device_count(int* count);
VK_API int vk_set_device(int device);
VK_API int vk_device_name(char* out, size_t bytes);

VK_API int vk_stream_create(void** stream);
VK_API int vk_stream_destroy(void* stream);
VK_API int vk_stream_synchronize(void* stream);   /* blocking */

/* Device memory for the host classes (ref: buffer.h:64-103, image.h:85-97). */
VK_API int vk_malloc(void** ptr, size_t bytes);
VK_API int vk_free(void* ptr);
VK_API int vk_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);  /* blocking */
VK_API int vk_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);  /* blocking */
VK_API int vk_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
VK_API int vk_memset(void* dst, int value, size_t bytes, void* stream);

/* Pinned, device-visible, coherent host memory (hipHostMalloc): the same pointer
 * is valid on the host and in kernels. Used for vk_track_poll.host_state. */
VK_API int vk_malloc_host(void** ptr, size_t bytes);
VK_API int vk_free_host(void* ptr);

/* Timing helpers (hipEvent) so hosts without HIP headers can time kernels. The
 * events carry no system-scope fence (hipEventDisableSystemFence): they order and
 * time work on a stream, they do not publish device writes to the host — use
 * vk_stream_synchronize or a blocking copy for that. */
VK_API int vk_event_create(void** event);
VK_API int vk_event_destroy(void* event);
VK_API int vk_event_record(void* event, void* stream);
VK_API int vk_event_elapsed_ms(void* start, void* stop, float* ms);  /* blocking on stop */

/* The input side of a frame (ref: include/vulcan/image.h:100-123 — Image::Load ends in a blocking cudaMemcpy —
 * called once per camera frame at apps/vulcan/vulcan.cu:220,232). Here a frame can be uploaded while the one
 * before it is being fused: the copy is enqueued on a stream of its own from pinned host memory (vk_malloc_host)
 * and returns at once; an ORDERING event (vk_event_create_ordering: no timing) recorded behind it is what the compute
 * stream waits for (vk_stream_wait_event) before the frame's first kernel, and an event recorded on the compute
 * stream behind the frame's last reader is what the copy stream waits for before it overwrites the image two frames
 * later. `publishes`: 1 when the work in front of the event WROTE what the waiter reads (the upload: default fences);
 * 0 when it only read what the waiter overwrites (the frame's kernels: no system-scope release — with one, every
 * record behind the integrate kernel wrote the device's caches back and the streamed frame took 357 us instead of
 * 114, tools/stream_input_probe.py). vk_event_synchronize blocks the HOST (before it refills a staging buffer).
 * vulcan_amd/host/include/vulcan/upload.h (FrameUploader) and bench.py --stream-input are built from these. */
VK_API int vk_memcpy_h2d_async(void* dst, const void* src_pinned, size_t bytes, void* stream);
VK_API int vk_event_create_ordering(void** event, int publishes);
VK_API int vk_stream_wait_event(void* stream, void* event);
VK_API int vk_event_synchronize(void* event);

/* ----------------------------------------------------------------- volume -- */

/* ref: src/volume.cu:552-627 Volume::Initialize + 9 Create* — fills voxels
 * with Voxel::Empty(), entries with HashEntry(), free list with 0..N-1,
 * types NONE, visibility FALSE; counters: visible=0, voxel_ptr=N-1,
 * excess_ptr=main. */
VK_API int vk_volume_initialize(const vk_volume* v, void* stream);

/* ref: src/volume.cu:465-471 Volume::ResetBlockVisibility — TRUE -> UNKNOWN */
VK_API int vk_volume_reset_block_visibility(const vk_volume* v, void* stream);

/* ref: src/volume.cu:87-301,497-518 Volume::CreateAllocationRequests.
 * One request per main bucket per call, as in the reference; where the
 * reference lets racing threads overwrite each other (last writer wins,
 * volume.cu:200,237) the winner here is the request with the largest packed
 * (pad=type,z,y,x) 64-bit key, chosen with one 64-bit atomic max, so a request
 * cannot tear and the outcome does not depend on timing. */
VK_API int vk_volume_create_allocation_requests(const vk_volume* v,
    const float* depth, int width, int height, const vk_projection* projection,
    const vk_transform* Twd, void* stream);

/* ref: src/volume.cu:304-368,520-535 Volume::HandleAllocationRequests.
 * Pool slots and excess indices are handed out in ascending bucket order
 * (an exclusive scan instead of the reference's atomicAdd/atomicSub order,
 * volume.cu:337,352), i.e. the outcome of running the reference's threads
 * serially; slot numbers are therefore reproducible. */
VK_API int vk_volume_handle_allocation_requests(const vk_volume* v, void* stream);

/* ref: src/volume.cu:25-84,473-495 Volume::UpdateBlockVisibility. Leaves the
 * count in counters[VK_CTR_VISIBLE]; does NOT read it back. The order of
 * visible_blocks is unspecified (as in the reference). */
VK_API int vk_volume_update_block_visibility(const vk_volume* v, int width,
    int height, const vk_projection* projection, const vk_transform* Tdw,
    void* stream);

/* ref: src/volume.cu:430-437 Volume::SetView = the four calls above. */
VK_API int vk_volume_set_view(const vk_volume* v, const vk_frame* frame, void* stream);

/* ref: src/volume.cu:537-543 Volume::GetBufferSize — blocking readback of the first
 * VK_CTR_PUBLIC counters into host memory (int32[VK_CTR_PUBLIC] or larger). */
VK_API int vk_volume_read_counters_sync(const vk_volume* v, int32_t* host_out, void* stream);

/* ------------------------------------------------------------- integrators -- */

/* Integrator parameters (ref: include/vulcan/integrator.h:38-44, integrator.cu:7-13) */
typedef struct vk_integrator {
  float min_depth;            /* depth_range_[0] = 0.1 */
  float max_depth;            /* depth_range_[1] = 5.0 */
  float max_distance_weight;  /* 16 */
  float max_color_weight;     /* 16 */
} vk_integrator;

/* ref: src/depth_integrator.cu:17-80,89-115 DepthIntegrator::Integrate
 * (= ColorIntegrator::IntegrateDepth color_integrator.cu:18-80,150-176
 *  = LightIntegrator::IntegrateDepth light_integrator.cu:106-168,295-321).
 * Visible blocks and their count are read from the volume on the device. */
VK_API int vk_integrate_depth(const vk_volume* v, const vk_integrator* p,
    const vk_frame* frame, void* stream);

/* ref: src/color_integrator.cu:83-135,178-204 ColorIntegrator::IntegrateColor */
VK_API int vk_integrate_color(const vk_volume* v, const vk_integrator* p,
    const vk_frame* frame, void* stream);

/* ref: src/color_integrator.cu:144-148 ColorIntegrator::Integrate — depth then
 * colour in ONE pass over the voxels (same values as the two reference passes:
 * the colour update reads the distance the depth update just wrote). */
VK_API int vk_integrate_depth_color(const vk_volume* v, const vk_integrator* p,
    const vk_frame* frame, void* stream);

/* ref: src/light_integrator.cu:17-103,277-293 LightIntegrator::ComputeFrameMask
 * (keeps the reference's asymmetric window). mask: [h*w] floats. */
VK_API int vk_light_compute_frame_mask(const vk_frame* frame, float depth_threshold,
    float* mask, void* stream);

/* ref: src/light_integrator.cu:277-293 LightIntegrator::ComputeFrameMask plus the part
 * of IntegrateColorKernel that depends on the PIXEL only (:215-225: the mask test and
 * the pixel's normal rotated into the colour camera, Tcd * n). `records`: device
 * float[h*w*4], 16-byte aligned, receives {Tcd * n (3), mask} per pixel, so the colour
 * kernel gathers one record per voxel instead of a mask and three normal components
 * and rotates nothing. `mask` is written as by vk_light_compute_frame_mask. Needs
 * frame->normals. */
VK_API int vk_light_prepare(const vk_frame* frame, float depth_threshold, float* mask,
    float* records, void* stream);

/* ref: src/light_integrator.cu:170-250,323-354 LightIntegrator::IntegrateColor */
VK_API int vk_integrate_light_color(const vk_volume* v, const vk_integrator* p,
    const vk_light* light, const float* mask, const vk_frame* frame, void* stream);

/* ref: src/light_integrator.cu:270-275 LightIntegrator::Integrate minus the
 * mask kernel: depth + light-colour update in one pass. */
VK_API int vk_integrate_depth_light(const vk_volume* v, const vk_integrator* p,
    const vk_light* light, const float* mask, const vk_frame* frame, void* stream);

/* ------------------------------------------------------------------ tracer -- */

/* ref: include/vulcan/tracer.cuh:14-18, src/tracer.cu:13-87,453-466
 * vulcan::ComputePatches. `block_count_dev` (device int*, may be NULL): when
 * non-NULL the number of visible blocks is read from it on the device and
 * `block_count` is only the upper bound used to size the grid. patch_count is
 * a device int the caller has zeroed (tracer.cpp:102-108). Patches are not
 * written past `patch_capacity`. Blocks with no valid depth interval emit no
 * patch (the reference writes patches[-1] there). */
VK_API int vk_trace_compute_patches(const int32_t* indices,
    const vk_hash_entry* entries, const vk_transform* Tcw,
    const vk_projection* projection, float block_length, float min_depth,
    float max_depth, int block_count, const int32_t* block_count_dev,
    int image_width, int image_height, int bounds_width, int bounds_height,
    vk_patch* patches, int patch_capacity, int32_t* patch_count, void* stream);

/* ref: tracer.cuh:20-21, src/tracer.cu:89-112,468-476 vulcan::ComputeBounds.
 * bounds: [bounds_h*bounds_w] float2 (near,far). patch_count_dev as above. */
VK_API int vk_trace_compute_bounds(const vk_patch* patches, float* bounds,
    int bounds_width, int patch_count, const int32_t* patch_count_dev, void* stream);

/* ref: tracer.cuh:32, src/tracer.cu:494-500 vulcan::ResetBoundsBuffer */
VK_API int vk_trace_reset_bounds(float* bounds, int count, void* stream);

/* Fused patches+bounds: every visible block rasterises its cell rectangle
 * straight into `bounds` (min/max are order independent, so the result is
 * bit-identical to ComputePatches + ComputeBounds). Resets bounds first. */
VK_API int vk_trace_compute_block_bounds(const int32_t* indices,
    const vk_hash_entry* entries, const vk_transform* Tcw,
    const vk_projection* projection, float block_length, float min_depth,
    float max_depth, int block_count, const int32_t* block_count_dev,
    int image_width, int image_height, int bounds_width, int bounds_height,
    float* bounds, void* stream);

/* ref: tracer.cuh:23-27, src/tracer.cu:114-451,478-492 vulcan::ComputePoints.
 * block_count = MAIN block count (the hash modulus K, tracer.cpp:85).
 * depths [h*w], colors [h*w*3]. */
VK_API int vk_trace_compute_points(const vk_hash_entry* entries,
    const vk_voxel* voxels, const float* bounds, int block_count,
    float block_length, float voxel_length, float trunc_length,
    const vk_transform* Twc, const vk_projection* projection, float* depths,
    float* colors, int image_width, int image_height, int bounds_width,
    int bounds_height, void* stream);

/* ref: tracer.cuh:29-30, src/frame.cu:9-122,183-192 vulcan::ComputeNormals
 * (= Frame::ComputeNormals frame.cpp:21-36). normals [h*w*3]. */
VK_API int vk_frame_compute_normals(const float* depths,
    const vk_projection* projection, float* normals, int image_width,
    int image_height, void* stream);

/* ref: src/frame.cu:126-181,194-203 vulcan::FilterDepths (7x7 bilateral). */
VK_API int vk_frame_filter_depths(int image_width, int image_height,
    const float* src, float* dst, void* stream);

/* Floats the `bounds` scratch of vk_trace must hold: the bounds grid itself
 * (tracer.cpp:140: 80*60 float2) followed by the per-workgroup private copies
 * the fused bounds pass reduces into and, since VK_ABI_VERSION 5, 2 048 words of
 * row counters for the raycast's normals (vk_trace_ahead_requests; one scratch
 * belongs to one vk_view_bounds record). */
VK_API size_t vk_trace_bounds_floats(int bounds_width, int bounds_height);

/* ref: src/tracer.cpp:41-47 Tracer::Trace — bounds (fused), points, normals.
 * `frame` supplies pose + intrinsics; outputs go to depth/color/normals
 * (all non-const device pointers owned by the caller). `bounds` is the
 * tracer's scratch, vk_trace_bounds_floats(w, h) floats; on return its first
 * w*h float2 hold the (near, far) grid of Tracer::bounds_. */
VK_API int vk_trace(const vk_volume* v, const vk_frame* frame, float min_depth,
    float max_depth, float* bounds, int bounds_width, int bounds_height,
    float* out_depth, float* out_color, float* out_normals, void* stream);

/* ------------------------------------------- light preparation, with SetView -- */

/* LightIntegrator's per-pixel preparation (vk_light_prepare: the frame mask and one
 * {Tcd * normal, mask} record per depth pixel) walks the depth image one lane per pixel,
 * exactly as the request pass of vk_volume_set_view does, and as a launch of its own most
 * of its ~6 us is the launch. An application that integrates the frame it has just set
 * the view from (the reference's frame loop, apps/vulcan/vulcan.cu:316-325) can have it
 * computed by that pass: vk_volume_set_view_prepare fills prep->mask / prep->records and
 * notes which frame they are for; the integrator asks (vk_light_prepared) and skips its
 * own pass on a match. "Which frame" means which CONTENT (vk_frame.content_id): upstream's
 * SetView reads the depth image only, so SetView(frame); frame.ComputeNormals();
 * Integrate(frame) is a legal sequence, and a preparation made before the normals changed
 * must not be used after. A frame whose content_id is 0 is never prepared ahead.
 * No reference counterpart; results are identical with or without it. */
typedef struct vk_light_prep {
  /* set by the caller */
  float  depth_threshold;      /* LightIntegrator::depth_threshold_ (light_integrator.cu:256) */
  float* mask;                 /* device float[capacity]                                       */
  float* records;              /* device float[4 * capacity], 16-byte aligned                  */
  /* One-shot request, reset to NULL by the call: the frame's normal image has NOT been computed yet
   * (Frame::ComputeNormals, frame.cu:9-122, still due) and vk_volume_set_view_prepare / _rounds is to
   * leave it in frame->normals — which this must equal — exactly as vk_frame_compute_normals would:
   * in its request pass when the preparation rides along (the 5-tap stencil reads the depth tile
   * that pass has staged anyway: one launch less per frame), else by that launch. */
  float* normals_out;
  int32_t capacity;            /* pixels the two buffers hold: a larger frame is not prepared  */
  /* set by vk_volume_set_view_prepare, compared by vk_light_prepared */
  int32_t      valid;
  int32_t      width, height;
  const float* depth;
  const float* color;
  const float* normals;
  float        prepared_threshold;
  vk_transform depth_to_color;
  uint64_t     content_id;     /* frame->content_id at the time; a frame with id 0 is never prepared */
} vk_light_prep;

/* ref: src/volume.cu:430-437 Volume::SetView (as vk_volume_set_view) + src/light_integrator.cu:
 * 277-293 — with a `prep` whose buffers are set and a frame that has colour and normals of
 * the depth image's size, the same launches also do vk_light_prepare. prep->valid
 * tells whether they did. (Two launches: the request pass; the handle pass and the visibility
 * pass together, the handle pass working from the list of buckets the request pass posted to.) */
VK_API int vk_volume_set_view_prepare(const vk_volume* v, const vk_frame* frame, vk_light_prep* prep,
    void* stream);

/* ref: apps/vulcan/vulcan.cu:316-318 — the frame loop calls SetView(frame) three times per frame,
 * because a bucket takes one request per call and a block that loses the contest for its bucket
 * (or finds its bucket's main entry taken by the winner) must ask again. This entry point leaves
 * exactly the state of `max_rounds` consecutive vk_volume_set_view(_prepare) calls with the same
 * frame — every buffer, the visible set, VK_CTR_VOXEL_PTR / EXCESS_PTR / REQUESTS / DROPPED — in the
 * two launches of ONE call. What a further call changes is only this: the blocks that lost ask
 * again, the winners among them are committed, their entries become visible. The request pass
 * therefore files the losers in a list, and — only when there are any — the workgroup of the second
 * launch that finishes last replays the later rounds from that list; the rays are walked once.
 * `prep` as in vk_volume_set_view_prepare (may be NULL). max_rounds >= 1. VK_CTR_ROUNDS counts the
 * rounds that ran; VK_CTR_UNSETTLED tells whether one more call would still have work.
 * Two cases end the rounds early, with VK_CTR_UNSETTLED = 1 and the state of as many calls as
 * rounds ran (VK_CTR_ROUNDS): a round that drops a request (pool or excess list exhausted —
 * upstream's calls after that link entries they never write, its state is inconsistent from
 * there on), and more than VK_RETRY_KEYS different blocks losing in one round. */
VK_API int vk_volume_set_view_rounds(const vk_volume* v, const vk_frame* frame, vk_light_prep* prep,
    int max_rounds, void* stream);

/* vk_volume_set_view_rounds with its two launches on two streams (round 4; no reference counterpart — upstream runs everything
 * on stream 0, device.h:40-52; ref: src/volume.cu:430-437 for the call). The request pass (volume.cu:497-518, with whatever rides in it: the light preparation, the
 * frame's normals) reads the depth image, the table and the visibility bytes and writes visibility bytes, request flags and
 * the preparation's buffers: nothing the raycast of the PREVIOUS frame reads or writes (vk_trace_ahead: table, voxels, its own
 * bounds and images). A caller that fuses at poses it knows before the previous frame's raycast has finished — the fusion +
 * raycast benchmark; not the tracking loop, whose pose comes out of that raycast — can therefore put the request pass on a stream
 * of its own and let it fill the tail of the previous raycast, whose last waves leave most of the device idle:
 *   vk_stream_wait_event(request_stream, integrated);   // the previous frame's vk_integrate_* has read the lists, mask, records
 *   vk_volume_set_view_rounds_split(&v, &f, &prep, 3, request_stream, ordering, stream);
 *   vk_integrate_ahead(.., stream);  vk_event_record(integrated, stream);  vk_trace_ahead(.., stream);
 * `ordering_event` (vk_event_create_ordering(&e, 1): the request pass WRITES what the waiter reads — visibility bytes, request
 * flags, the posted list, the preparation's buffers, the normals — so the event is one that publishes; `integrated` above is
 * vk_event_create_ordering(&e, 0): the integrate launch only read what the request pass overwrites) is recorded behind the
 * request pass on request_stream, and `stream` waits
 * for it before the handle + visibility pass, which must follow the previous raycast anyway (it writes table entries).
 * Same state as vk_volume_set_view_rounds, bit for bit (tests/test_gpu_configs.py runs bench.py's step, which uses this). */
VK_API int vk_volume_set_view_rounds_split(const vk_volume* v, const vk_frame* frame, vk_light_prep* prep, int max_rounds,
    void* request_stream, void* ordering_event, void* stream);

/* ref: src/light_integrator.cu:270-275 LightIntegrator::Integrate decides here whether
 * ComputeFrameMask still has to run: 1 if *prep holds the preparation of exactly `frame` (same
 * non-zero content_id, same image pointers and size, same depth->colour transform) at
 * `depth_threshold`, else 0. */
VK_API int vk_light_prepared(const vk_light_prep* prep, const vk_frame* frame, float depth_threshold);

/* ---------------------------------------------------- raycast bounds, ahead -- */

/* The first stage of a raycast (per-cell depth bounds of the visible blocks,
 * tracer.cpp:49-76) depends only on the visible list and the view, not on the
 * voxels, and it is a short latency-bound pass that keeps a few CUs busy. An
 * application that raycasts from the pose it has just integrated (the reference's
 * frame loop, apps/vulcan/vulcan.cu:316-325) can have it computed by a handful of
 * extra workgroups INSIDE the integrate launch, where it costs nothing, and let
 * the raycast skip it. This record carries the result and the view it is for.
 * No reference counterpart; results are identical with or without it. */
typedef struct vk_view_bounds {
  /* set by the caller */
  float*        scratch;          /* device, vk_trace_bounds_floats(bounds_width, bounds_height) floats */
  int32_t       bounds_width;     /* the tracer's grid (80 x 60, tracer.cpp:108-111) */
  int32_t       bounds_height;
  float         min_depth;        /* the tracer's depth range (tracer.cpp:103-106)   */
  float         max_depth;
  /* set by vk_integrate_ahead / vk_trace_ahead, compared by vk_trace_ahead. The
   * caller zeroes `valid` whenever the visible list changes: after
   * vk_volume_set_view and after the staged visibility calls. */
  int32_t       valid;
  int32_t       width, height;
  float         block_length;
  const void*   visible_blocks;   /* which volume */
  vk_projection projection;
  vk_transform  depth_to_world;
  /* kept by vk_trace_ahead / vk_trace_ahead_requests (the caller only zeroes them with the record): the raycast's normals
   * are computed by trailing workgroups of the SAME launch, which wait per 8-pixel row of tiles for the counters behind
   * the bounds in `scratch`; these say for which scratch and image size the counters count, and how many launches far */
  const float*  counted_scratch;
  int32_t       counted_width, counted_height;
  uint32_t      trace_launches;
  int32_t       pad_;
  /* (ABI 6) The waiting normals workgroups' wait is BOUNDED (a launch whose counters were left behind by an aborted
   * one must not hang the device). A group whose wait expires stores nothing, sets a word behind the counters in
   * `scratch` and — when the caller gave one — `*late_host`: one int32 of pinned host memory (vk_malloc_host), zeroed by
   * the caller once; the value stored is the number of the launch (1, 2, ... as this record counts them since its counters
   * were last zeroed, never 0) whose group expired (round 6). The library looks at it, without synchronising anything, at the start of every vk_trace_ahead* call
   * with this record, and vk_trace_normals_settle does after synchronising; see there for what happens then. The
   * `last_*` fields say which images the riding normals of the last launch belong to (set by the library).
   * ONE stream at a time per record: the counters' target counts the launches in stream order, so two traces in
   * flight on two streams through one record would wait for the wrong count. A call that names another stream than the
   * last one re-zeroes the counters on the new stream — the caller makes sure the old stream's launch has completed. */
  int32_t*      late_host;
  const float*  last_depths;
  float*        last_normals;
  int32_t       last_width, last_height;
  vk_projection last_projection;
  const void*   counted_stream;
} vk_view_bounds;

/* vk_integrate_depth / _depth_color / _depth_light (color_mode 0 / 1 / 2; `light`
 * and `mask` as in vk_integrate_depth_light for mode 2; `light_records`: optional
 * output of vk_light_prepare for the same frame, NULL = gather mask and normals
 * separately) which, when `ahead` is given, also computes the raycast bounds of
 * `frame`'s own view into ahead->scratch and records the view in *ahead.
 * ref: as those three. */
VK_API int vk_integrate_ahead(const vk_volume* v, const vk_integrator* p,
    const vk_frame* frame, int color_mode, const vk_light* light, const float* mask,
    const float* light_records, vk_view_bounds* ahead, void* stream);

/* A measurement aid (round 5; no reference counterpart — upstream times nothing on the device; ref: src/depth_integrator.cu:
 * 83-120, src/light_integrator.cu:296-340 for the launches it times): the NEXT pipelined integrate launch issued from this
 * host thread (vk_integrate_depth / _depth_color / _depth_light / vk_integrate_ahead) records `start_event` and `stop_event`
 * (vk_event_create) as the begin and the end OF THE DISPATCH ITSELF (hipExtLaunchKernelGGL) — the duration rocprofv3's kernel
 * trace reports. A caller that brackets the call with two vk_event_record instead also times the events' own processing and
 * the launch latency behind the first of them: 1.7 - 3.5 us on a 34 us launch, which is what separated bench.py's roofline
 * fraction from the kernel trace's until round 5. One CALL only: the pair is used up by the next vk_integrate_* call of this
 * thread even when that call returns an error before its launch (round 6: events left armed by a failed call were recorded by a
 * later, unrelated launch); (NULL, NULL) cancels. Not a stream operation: nothing is enqueued by this call. */
VK_API int vk_integrate_time_next(void* start_event, void* stop_event);

/* ref: src/tracer.cpp:41-47 Tracer::Trace, as vk_trace with the grid, depth range
 * and scratch taken from *ahead: when *ahead holds the bounds of this very view
 * the bounds pass is skipped, otherwise it runs and *ahead is updated. `normals` may be NULL (round 5): the normal image is
 * then left to the caller — e.g. to the next frame's vk_icp_pyramid_track_frame(.., frame_normals_due = 2 | .., ..). */
VK_API int vk_trace_ahead(const vk_volume* v, const vk_frame* frame,
    vk_view_bounds* ahead, float* depths, float* colors, float* normals, void* stream);

/* The request pass of a frame's SetView done AHEAD, in the previous frame's raycast launch (round 4; no reference
 * counterpart; ref: src/volume.cu:430-437,497-518 and src/tracer.cpp:41-47 for the two calls it joins). A raycast launch is as
 * long as its slowest wave and leaves most of the device idle for its last third; the request pass of the NEXT frame reads
 * and writes nothing the raycast touches (see vk_volume_set_view_rounds_split), so for a caller that knows the next frame — its
 * images and its pose — when it raycasts this one (fusion at given poses; not the tracking loop, whose next pose comes out of
 * this raycast) the pass can ride behind the raycast's workgroups in the SAME launch:
 *   vk_trace_ahead_requests(&v, &key_i, &bounds, depth, color, normals, &frame_next, &prep, &ahead, stream);   // Trace(i) + requests(i+1)
 *   ...
 *   vk_volume_set_view_rounds_ahead(&v, &frame_next, &prep, 3, &ahead, stream);    // SetView(i+1): the handle + visibility pass only
 * `ahead` is a caller-owned record (zero it once) that names the frame the pass was made for; vk_volume_set_view_rounds_ahead
 * uses the pass only for that very frame (same volume, images, size, intrinsics, pose and non-zero content_id, same riding
 * preparation); with a record that is not valid (zeroed, already used, or vk_trace_ahead_requests could not make the pass:
 * no content_id, normals asked for without a riding preparation) it runs the whole call, so the outcome is
 * vk_volume_set_view_rounds', bit for bit (tests/test_gpu_configs.py runs bench.py's step, which uses this). A VALID record
 * for another frame is refused (VK_ERR_ARGUMENT, nothing launched, the record kept): that frame's requests are in the volume,
 * and handled together with this frame's they would allocate in an order no sequence of upstream calls gives — the announced
 * frame has to be fused first. Between the two calls nothing else may run a SetView stage on the volume. `next_prep` as in vk_volume_set_view_prepare (may be NULL): the light preparation — and, with normals_out, the
 * next frame's normals — ride with the pass as they do in SetView. */
typedef struct vk_requests_ahead {
  const void*   counters;          /* the volume the pass was made on */
  const float*  depth;
  const void*   prep;              /* the vk_light_prep that rode along, or NULL */
  int32_t       width, height;
  vk_projection depth_projection;
  vk_transform  depth_to_world;
  uint64_t      content_id;
  int32_t       valid;
  int32_t       normals_made;      /* round 6 (was padding): 1 = the announced frame's normal image (next_frame->normals) was written
                                      with the pass (next_prep->normals_out rode) — or, set by the class layer, by a launch of its
                                      own in front of the announce; 0 = the announce left the normals as they were. A caller
                                      whose next step is "ComputeNormals, then SetView" may skip the normals only on 1 */
  int32_t       pose_on_device;    /* round 6: 1 = the pass was made by vk_volume_requests_at_device_pose — at the pose a tracker had
                                      left on the device, which the host did not have yet; vk_volume_set_view_rounds_ahead then takes
                                      the frame's pose on trust (the caller read it from that same device pose), and depth_to_world
                                      above is the Track's START pose (what vk_requests_ahead_cancel completes after an aborted Track) */
  int32_t       pad_;
} vk_requests_ahead;

VK_API int vk_trace_ahead_requests(const vk_volume* v, const vk_frame* view, vk_view_bounds* ahead, float* out_depth,
    float* out_color, float* out_normals, const vk_frame* next_frame, vk_light_prep* next_prep,
    vk_requests_ahead* requests, void* stream);
VK_API int vk_volume_set_view_rounds_ahead(const vk_volume* v, const vk_frame* frame, vk_light_prep* prep, int max_rounds,
    vk_requests_ahead* requests, void* stream);

/* The request pass of a TRACKED frame's SetView without the host round trip in front of it (round 6; no reference counterpart;
 * ref: src/volume.cu:430-437,497-518 Volume::SetView's first stage, apps/vulcan/vulcan.cu:300-318 for the loop). In the tracking
 * loop the pose of frame i comes out of Tracker::Track, the host waits for it (Tracker::EndSolve), and only then can it enqueue
 * SetView / Integrate / Trace — which need the pose as launch arguments: the device idles for the round trip, ~15 us of a 272 us
 * frame (profiles/r06_tracked_frame_timeline.txt). The request pass is the first launch behind that gap, and it needs the pose
 * for nothing but the rays' origin and direction: here it takes them from *pose_dev — the vk_transform the tracker's launches in
 * front of it in `stream` leave on the device (vk_icp_track*'s Twc_dev) — so the host enqueues it RIGHT BEHIND the Track, before
 * it waits, and has the whole pass (19 us) to pick up the pose and enqueue the rest:
 *   vk_icp_pyramid_track_frame(.., Twc_dev, .., stream);                                 // Track(i), enqueued
 *   vk_volume_requests_at_device_pose(&v, &frame, Twc_dev, &prep, &record, stream);      // requests(i), enqueued: no wait
 *   vk_track_wait(&poll, stream);  frame.depth_to_world = *poll.host_pose;               // Tracker::EndSolve
 *   vk_volume_set_view_rounds_ahead(&v, &frame, &prep, 3, &record, stream);              // handle + visibility only
 * `frame`: as for vk_volume_set_view_prepare, its depth_to_world = the Track's start pose (ignored by the pass; kept in the
 * record for vk_requests_ahead_cancel). `prep` rides as in SetView (the frame's normals must exist: normals_out is refused,
 * VK_ERR_UNSUPPORTED). The same requests as SetView's own pass at the pose the host then reads: the same state, bit for bit
 * (tests/test_gpu_round6.py). A Track that ends with VK_TRACK_ABORTED has left its start pose in *pose_dev: the record then
 * announces a SetView at the start pose — vk_requests_ahead_cancel completes it (a state upstream reaches by calling SetView
 * with the untracked frame), after which the staged Track and the frame's own SetView follow. */
VK_API int vk_volume_requests_at_device_pose(const vk_volume* v, const vk_frame* frame, const vk_transform* pose_dev,
    vk_light_prep* prep, vk_requests_ahead* requests, void* stream);

/* ref: src/volume.cu:430-437 Volume::SetView (x max_rounds, as vk_volume_set_view_rounds) — the WHOLE call at the pose on the
 * device: the request pass as above and the handle + visibility launch with its frustum test's world -> depth transform taken
 * from pose_dev->inv. Nothing of SetView then waits for the host: a tracking loop enqueues it right behind the Track and has
 * both launches (28 us) to pick the pose up (vk_track_wait) for Integrate and Trace — which found the device idle for 6 us even
 * behind the request pass alone (profiles/r06_tracked_frame_timeline.txt). `frame->depth_to_world` is ignored. No record: there
 * is no later SetView call to match. After a Track that ABORTED the volume has seen SetView(frame at the Track's start pose) —
 * a state upstream reaches — and the caller's staged Track and the frame's own SetView follow. VK_ERR_UNSUPPORTED (nothing
 * launched): prep->normals_out set, or vk_test_hooks.set_view_unfused. Same state as vk_volume_set_view_rounds with the pose
 * the host then reads, bit for bit (tests/test_gpu_round6.py). */
VK_API int vk_volume_set_view_at_device_pose(const vk_volume* v, const vk_frame* frame, const vk_transform* pose_dev,
    vk_light_prep* prep, int max_rounds, void* stream);

/* A record that is still valid when vk_trace_ahead_requests is called again names a frame whose requests are in the volume
 * and whose SetView has not run: a second pass on top would mix two frames' requests, retry keys, posted list and touched
 * bits — the state vk_volume_set_view_rounds_ahead refuses. vk_trace_ahead_requests therefore returns VK_ERR_ARGUMENT for a
 * record with valid == 1 and launches nothing (round 5), and the staged SetView stages of the class layers refuse to run
 * while their volume's record is valid. The way out of such a record — one a SetView refused, or a frame the caller no
 * longer wants to fuse — is this call: it completes the ANNOUNCED frame's SetView (the handle + visibility pass with the
 * record's own size, intrinsics and pose: everything that pass needs; `max_rounds` as there) and marks the record used. The
 * volume is then exactly where `max_rounds` upstream SetView calls with the announced frame leave it — a state upstream can
 * reach — and any frame may follow. A record that is not valid: VK_OK, nothing launched. A record of another volume:
 * VK_ERR_ARGUMENT. ref: src/volume.cu:430-437 (the SetView it completes), :520-535, :473-495. */
VK_API int vk_requests_ahead_cancel(const vk_volume* v, vk_requests_ahead* requests, int max_rounds, void* stream);

/* The outcome of the bounded wait of the raycast's riding normals (vk_view_bounds.late_host; round 5; no reference
 * counterpart; ref: include/vulcan/device.h:14-17 CUDA_ASSERT — the contract it keeps is upstream's "a failed device step
 * always surfaces" — and src/frame.cu:9-122 for the normals it recomputes). Synchronises `stream`, then looks at the expiry word (the pinned one,
 * or — without one — the word behind the counters, by a blocking copy). Nothing expired: VK_OK. Otherwise the riding
 * normals of A launch since the last check are incomplete: the stream the counters counted on is drained, the counters and
 * both words are re-zeroed, the launch count starts over, Frame::ComputeNormals of the LAST traced image is enqueued on
 * `stream` as a launch of its own (ahead->last_*), and the call returns VK_ERR_TIMEOUT. What is guaranteed is the error: the
 * caller knows its counters had been left in a bad state. The image repaired is the most recent one; a caller that runs
 * several launches ahead of this check and kept an EARLIER image (the pinned word held the number of the launch that
 * expired until this call zeroed it) recomputes that image's normals itself (vk_frame_compute_normals). Every vk_trace_ahead / vk_trace_ahead_requests call makes the same check first, on the pinned word
 * only and without synchronising; when it finds the word set it repairs in the same way, launches NOTHING of its own and
 * returns VK_ERR_TIMEOUT — the caller repeats the call. */
VK_API int vk_trace_normals_settle(vk_view_bounds* ahead, void* stream);

/* ------------------------------------------------------------------- image -- */

/* ref: src/image.cu:101-165,183-211 Image::Downsample (nearest or 2x2 box). dst is (src_w / 2) x (src_h / 2),
 * rounded down: an odd size loses its last column / row, which is what upstream's kernels compute (its host
 * wrapper asks for even sizes in debug builds only); nothing is launched for an empty dst. The same holds for
 * vk_color_image_downsample and vk_frame_downsample. */
VK_API int vk_image_downsample(int src_w, int src_h, const float* src,
    float* dst, int nearest, void* stream);

/* ref: src/image.cu:133-165,234-262 ColorImage::Downsample */
VK_API int vk_color_image_downsample(int src_w, int src_h, const float* src,
    float* dst, int nearest, void* stream);

/* ref: src/frame.cpp:38-51 Frame::Downsample's three image passes in one launch: depth and
 * normals nearest, colour 2x2 box (exactly vk_image_downsample / vk_color_image_downsample).
 * An output that is NULL is skipped; depth and normals have the size frame->width x height,
 * the colour image its own (color_width x color_height, 0 = the same). */
VK_API int vk_frame_downsample(const vk_frame* frame, float* depth_out, float* color_out,
    float* normals_out, void* stream);

/* --------------------------------------------------------------------- ICP -- */

/* One side of the ICP problem (keyframe or frame). */
typedef struct vk_icp_view {
  const float*  depths;      /* [h*w]   */
  const float*  normals;     /* [h*w*3] */
  int32_t       width;
  int32_t       height;
  vk_projection projection;
} vk_icp_view;

/* ref: src/depth_tracker.cu:97-118,272-300 DepthTracker::ComputeResiduals */
VK_API int vk_icp_compute_residuals(const vk_icp_view* keyframe,
    const vk_transform* Twm, const vk_icp_view* frame, const vk_transform* Twc,
    float* residuals, void* stream);

/* ref: src/depth_tracker.cu:120-141,302-336 DepthTracker::ComputeJacobian.
 * jacobian: [h*w*6] floats; columns 3..5 are 0 when !translation_enabled. */
VK_API int vk_icp_compute_jacobian(const vk_icp_view* keyframe,
    const vk_transform* Twm, const vk_icp_view* frame, const vk_transform* Twc,
    int translation_enabled, float* jacobian, void* stream);

/* ref: src/depth_tracker.cu:144-268,338-378 DepthTracker::ComputeSystem.
 * hessian: device float[36] — the first 21 (6 when !translation_enabled) hold
 * the packed lower triangle, row-major (r, c<=r), rest zero; gradient: device
 * float[6]. Both are overwritten (the reference zero-fills then atomically
 * accumulates; this is a two-stage fixed-order reduction, so the sums are
 * reproducible). `workspace`: device float[vk_icp_workspace_floats(w,h)].
 * `Twc_dev`: optional DEVICE pointer to a vk_transform that overrides Twc
 * (lets a device-side Gauss-Newton loop run without host round trips). */
VK_API size_t vk_icp_workspace_floats(int width, int height);
VK_API int vk_icp_compute_system(const vk_icp_view* keyframe,
    const vk_transform* Twm, const vk_icp_view* frame, const vk_transform* Twc,
    const vk_transform* Twc_dev, int translation_enabled, float* workspace,
    float* hessian, float* gradient, void* stream);

/* ref: src/tracker.cpp:124-163 Tracker::ComputeUpdate + src/depth_tracker.cpp:
 * 22-86 DepthTracker::ApplyUpdate, on the device: unpack the packed lower
 * triangle, LDLT-solve x = -H^-1 g, compose Tinc*Twc, re-orthonormalise, write
 * the new transform to *Twc_dev. state_dev: device int[2] = {iteration, done};
 * once ||x|| < 1e-6 (tracker.cpp:162) `done` is set and later calls become
 * no-ops (the pose stops changing), so a fixed-length device-side loop gives
 * the same pose as the reference's early exit.
 * update_dev (optional): device float[6] receiving x. */
VK_API int vk_icp_solve_update(const float* hessian, const float* gradient,
    int translation_enabled, vk_transform* Twc_dev, int32_t* state_dev,
    float* update_dev, void* stream);

/* ref: src/tracker.cpp:124-163 Tracker::ComputeUpdate + src/depth_tracker.cpp:22-86 DepthTracker::ApplyUpdate for ONE
 * CAMERA OF A RIGID RIG (see "A rigid multi-camera rig" below; the reference has one camera): the same solve and the
 * same Tinc as vk_icp_solve_update, applied as *Twc_dev = rigid_from(D * Twc) with D = rigid_from(Tinc), the
 * re-orthonormalisation of Tinc alone — a rigid motion that does not depend on the camera it is applied to. Every
 * other argument, `state_dev` and the no-op after convergence as in vk_icp_solve_update. */
VK_API int vk_icp_solve_update_rig(const float* hessian, const float* gradient,
    int translation_enabled, vk_transform* Twc_dev, int32_t* state_dev,
    float* update_dev, void* stream);

/* Called between the system and the solve of every iteration with the packed
 * device system (48 floats: hessian[36], gradient[6], pad): a multi-GPU rig sums
 * it over ranks here (ncclAllReduce on `stream`). Returns 0 on success. */
typedef int (*vk_icp_reduce_fn)(float* system_dev, int count, void* user, void* stream);

/* A reduce hook that changes nothing. Passing it selects the launch-per-stage loop of a tracker
 * on one GPU (ref: src/tracker.cpp:53-63, one ComputeSystem + ComputeUpdate per iteration): what a
 * host falls back to when a one-launch loop ends with VK_TRACK_ABORTED. */
VK_API int vk_reduce_nothing(float* system_dev, int count, void* user, void* stream);

/* *dst_dev = *src_host, stream-ordered and without a host synchronisation (the 128
 * bytes travel as kernel arguments): how a tracker's device-side pose is seeded
 * from frame.depth_to_world_transform (ref: src/tracker.cpp:70-76 BeginSolve). */
VK_API int vk_transform_upload(vk_transform* dst_dev, const vk_transform* src_host, void* stream);

/* Early exit for the device-side Gauss-Newton loops. The reference leaves its loop
 * as soon as |update| < 1e-6 (tracker.cpp:162) because its host sees every update.
 * The loops here are enqueued without a host round trip; steps after convergence
 * are no-ops but still cost their launches. With a vk_track_poll the solve also
 * publishes {iterations, converged} to `host_state` (ONE 64-bit store to pinned host
 * memory, vk_malloc_host), and the enqueuing function looks at it after every
 * `chunk` steps and stops once the loop has converged: the pose is the same, the
 * call blocks for at most one chunk, and no launch follows convergence by more
 * than 2 * chunk - 1 steps. The number of steps enqueued depends only on the step at
 * which the loop converged — not on timing — so all ranks of a multi-GPU rig (whose
 * steps carry an all-reduce each) enqueue the same number. NULL (or chunk <= 0):
 * enqueue every step, never block. */
typedef struct vk_track_poll {
  int32_t* host_state;   /* pinned int32[4], 8-byte aligned, zeroed once by the caller: [0..1] the
                            device's word {steps, converged | call tag}, [2] the library's call counter,
                            [3] the tag of the last call whose pose has arrived in host_pose             */
  int32_t  chunk;        /* steps enqueued between two looks at host_state (0: never look)               */
  vk_transform* host_pose;  /* optional, pinned (vk_malloc_host): every Track also leaves its final pose
                            here (for the colour trackers: depth_to_world); see vk_track_wait            */
} vk_track_poll;

/* ref: src/tracker.cpp:78-82 Tracker::EndSolve — the pose of the last Track issued with `poll` is in
 * poll->host_pose when this returns VK_OK. It watches one word of pinned memory that the last kernel
 * of the Track writes after the pose (a few microseconds after the kernel is done) instead of copying
 * the pose and synchronising the stream. VK_ERR_UNSUPPORTED: `stream` drained without the pose having
 * been left (a Track that failed, or none was issued with this `poll`). */
VK_API int vk_track_wait(const vk_track_poll* poll, void* stream);

/* ref: src/tracker.cpp:53-63 Tracker::Track for DepthTracker — up to `iterations`
 * Gauss-Newton steps without a host round trip, ending early once |update| < 1e-6
 * (tracker.cpp:162). `system`: device float[48]; `state_dev`: device int[2]
 * {steps run, converged}, the caller zeroes it (a state that says "converged" makes
 * the call a no-op); `workspace`: vk_icp_workspace_floats(w, h) floats.
 *
 * Without a `reduce` hook the whole loop is ONE launch: the workgroups exchange
 * their 27 sums inside the launch after every step, each adds all of them in a fixed
 * order and solves the 6x6 system itself (redundantly, hence identically), workgroup 0
 * publishes pose, system and state at the end (a loop of more than 32 steps continues in
 * further launches of 32). `poll` is not
 * needed for an early exit on this path (its mirror still receives the final state).
 * Should the device be unable to hold the launch's workgroups at the same time — not
 * expected: the grid is sized from the occupancy query — the launch gives up after two
 * seconds and leaves state_dev[1] = VK_TRACK_ABORTED; no pose is published then (vk_track_wait
 * returns VK_ERR_UNSUPPORTED), a later level of the same coarse-to-fine Track does not run,
 * and the host's way out is the same call again from the start pose with `reduce` =
 * vk_reduce_nothing, i.e. the launch-per-stage loop, which waits for nobody (the class layer and
 * vulcan_amd/api.py do exactly that). With vk_test_hooks.loop_cooperative set the loop
 * kernels are launched with hipLaunchCooperativeKernel, which refuses a grid that cannot be
 * resident instead of letting the kernel find out. Tracks issued on different streams of
 * one device are run one after the other by the library (a loop launch fills the device); two
 * processes that share a device are not protected from starving each other.
 *
 * With a `reduce` hook (multi-GPU rig) a step is three launches — partial sums, sum,
 * [the hook's all-reduce], solve — and `poll` stops the enqueuing after convergence. */
#define VK_TRACK_ABORTED (-1)
VK_API int vk_icp_track(const vk_icp_view* keyframe, const vk_transform* Twm,
    const vk_icp_view* frame, vk_transform* Twc_dev, int iterations,
    int translation_enabled, float* workspace, float* system, int32_t* state_dev,
    float* update_dev, vk_icp_reduce_fn reduce, void* reduce_user, const vk_track_poll* poll,
    void* stream);

/* A rigid multi-camera rig, one camera per GPU (BASELINE configs[4]; no reference counterpart): the
 * ranks' views contribute to ONE normal system, so after every rank has summed its own view the 27
 * sums are added over ranks and every rank runs the same solve. With `reduce` that costs three
 * launches and an all-reduce per Gauss-Newton step; with a vk_rig_exchange the one-launch loop is
 * kept: one workgroup of every rank writes its 27 {tag, value} words straight into every peer's
 * memory (areas mapped over xGMI by vk_comm_exchange_attach, include/vk_comm.h), all workgroups
 * read their own GPU's area, add the ranks' words in rank order (the same bits everywhere) and
 * solve. Protocol and its proof obligations: vulcan_amd/csrc/vk_rig_protocol.h.
 *
 * THE RIG'S INCREMENT. The update x of the one solve must move every camera by the SAME world-frame
 * rigid motion, or the rig bends. DepthTracker::ApplyUpdate (src/depth_tracker.cpp:33-84) does not
 * do that when it is run per camera: Tinc(1,2) = +x[0] (upstream's sign, kept: SURVEY 2.5-11) makes
 * Tinc no rotation to first order, and what the re-orthonormalisation of Tinc * Twc makes of its
 * symmetric part depends on Twc. Cameras that are not parallel or opposed drift apart by O(|x[0]|)
 * in the first steps, nothing in the common solve can pull them back, and the loop converges on a
 * rig that is bent — 6 to 8 mm and 0.4 degrees for the ring of configs[4] from a 5 mm start
 * (docs/rounds/r08.md; oracle: oracle.rig_track, tests/test_oracle_rig.py). The rig's Tracks therefore
 * apply D = rigid_from(Tinc), Gram-Schmidt of Tinc alone — exp([x]) to first order, independent of
 * the pose — as Twc_r = rigid_from(D * Twc_r):
 *   vk_icp_track_rig with world > 1, vk_icp_track_rig_hook, vk_icp_solve_update_rig.
 * Everything else keeps ApplyUpdate as upstream has it (the "camera form"), bit for bit: vk_icp_track
 * with or without a `reduce` hook (a hook alone does not make a rig: vk_reduce_nothing is the fallback
 * of plain Tracks), vk_icp_track_rig with world == 1, vk_icp_solve_update, and every
 * vk_icp_pyramid_track* call — their `reduce` argument runs the camera form, so a rig that tracks
 * coarse-to-fine through them is only right for parallel or opposed cameras. */
#define VK_RIG_MAX_RANKS 8
typedef struct vk_rig_exchange {
  unsigned long long* areas[VK_RIG_MAX_RANKS]; /* areas[r]: rank r's area as mapped into THIS process (areas[rank]:
                                                  its own); each of the size vk_rig_area_bytes returns, zeroed once, fine-grained */
  int32_t  rank, world;
  uint32_t sequence;      /* names the Track: the same on every rank, 22 bits, never 0; after EVERY Track it entered
                             (an aborted one too) a rank moves it on with vk_comm_exchange_next_sequence
                             (vk_comm.h): 1, 2, ... 2^22 - 2, 1, ... — the parity alternates across the wrap */
} vk_rig_exchange;

/* bytes of one rank's area (ref: none — the reference has no multi-GPU code) */
VK_API size_t vk_rig_area_bytes(void);

/* ref: src/tracker.cpp:53-63 Tracker::Track for DepthTracker on a rig: vk_icp_track (no `reduce`: the whole
 * loop is one launch per rank) with the ranks' sums added through `rig` after every step. Every rank
 * calls it for the same Track with the same sequence number, iterations (<= 1000) and
 * translation_enabled. world > 1 applies the rig's increment (above); world == 1 gives vk_icp_track's bits.
 * A rank that waits two seconds for a peer ends with VK_TRACK_ABORTED. */
VK_API int vk_icp_track_rig(const vk_icp_view* keyframe, const vk_transform* Twm,
    const vk_icp_view* frame, vk_transform* Twc_dev, int iterations,
    int translation_enabled, float* workspace, float* system, int32_t* state_dev,
    float* update_dev, const vk_rig_exchange* rig, const vk_track_poll* poll, void* stream);

/* ref: src/tracker.cpp:53-63 Tracker::Track for DepthTracker on a rig whose sums are added by a `reduce` hook
 * (required: an all-reduce over the ranks, e.g. vk_comm_reduce_hook): vk_icp_track with that hook — three launches
 * per step, `poll` stops the enqueuing after convergence — whose solve applies the rig's increment (above). The
 * opt-in of the hook path: vk_icp_track itself keeps the camera form whatever `reduce` is. Arguments as vk_icp_track. */
VK_API int vk_icp_track_rig_hook(const vk_icp_view* keyframe, const vk_transform* Twm,
    const vk_icp_view* frame, vk_transform* Twc_dev, int iterations,
    int translation_enabled, float* workspace, float* system, int32_t* state_dev,
    float* update_dev, vk_icp_reduce_fn reduce, void* reduce_user, const vk_track_poll* poll,
    void* stream);

/* ref: src/pyramid_tracker.cpp:52-90 PyramidTracker<DepthTracker>::Track — the half-
 * resolution level of both frames (Frame::Downsample, src/frame.cpp:38-58: nearest
 * depth and normals, intrinsics / 2; ONE launch for the four images), vk_icp_track
 * with 15 steps on it, then 20 steps at full resolution from the pose the half
 * level left (one launch per level when there is no `reduce` hook). The quarter level
 * upstream builds and never tracks (:64-77) is not built. `pyramid`: device float[vk_icp_pyramid_floats(...)] for the half-resolution
 * images; `workspace`: vk_icp_workspace_floats of the FULL frame size; the other
 * buffers as in vk_icp_track. state_dev is reset before each level and holds the
 * full-resolution level's {steps, converged} afterwards. Image sizes must be even.
 * `reduce` runs both levels launch per stage with the CAMERA form of the pose update (vk_icp_track's), also when the
 * hook sums over the ranks of a rig: there is no coarse-to-fine rig Track yet ("THE RIG'S INCREMENT" above). */
VK_API size_t vk_icp_pyramid_floats(int key_width, int key_height, int frame_width, int frame_height);
VK_API int vk_icp_pyramid_track(const vk_icp_view* keyframe, const vk_transform* Twm,
    const vk_icp_view* frame, vk_transform* Twc_dev, float* pyramid, float* workspace,
    float* system, int32_t* state_dev, float* update_dev, vk_icp_reduce_fn reduce,
    void* reduce_user, const vk_track_poll* poll, void* stream);

/* vk_icp_pyramid_track for the frame loop (apps/vulcan/vulcan.cu:297-311: frame.ComputeNormals(); tracker->Track(frame)), with
 * two launches of that sequence folded into the pyramid's own: `Twc_start` (host, may be NULL) is stored to Twc_dev by the
 * pyramid launch (instead of vk_transform_upload before the call), and with `frame_normals_due` the frame's normal image
 * frame->normals is COMPUTED by it (ref: src/frame.cu:9-122 Frame::ComputeNormals — vk_frame_compute_normals' bits; the
 * half-resolution normals are computed at the pixels they are sampled from, which is the same normal) instead of read.
 * `frame_normals_due` is a set of bits: 1 = the frame's normal image as above; 2 (round 5) = the KEYFRAME's — the raycast's
 * normal image, which Tracer::Trace otherwise computes with a launch of its own right behind the raycast (src/tracer.cpp:97-100)
 * and which nobody reads before this Track: vk_trace_ahead(.., normals = NULL, ..) leaves it out, and this call writes
 * keyframe->normals (the same bits) on the way. The caller that skips the raycast's normals owes them to whoever reads the
 * key frame before the next Track. Everything else as vk_icp_pyramid_track. */
VK_API int vk_icp_pyramid_track_frame(const vk_icp_view* keyframe, const vk_transform* Twm,
    const vk_icp_view* frame, vk_transform* Twc_dev, const vk_transform* Twc_start, int frame_normals_due,
    float* pyramid, float* workspace, float* system, int32_t* state_dev, float* update_dev,
    vk_icp_reduce_fn reduce, void* reduce_user, const vk_track_poll* poll, void* stream);

/* The NEXT Track's pyramid behind the raycast (round 6) was measured to lose and is retired: tools/patches/README.md names
 * the last commit that builds it. Both calls stay for ABI-7 callers and never ride. vk_trace_ahead_pyramid checks its
 * arguments (all sizes even), leaves *built invalid and is vk_trace_ahead(v, frame, ahead, depths, colors, normals):
 * next_frame and `pyramid` are not written. vk_icp_pyramid_track_built clears *built and is vk_icp_pyramid_track_frame. */
typedef struct vk_pyramid_ahead {
  const float* key_depths;     /* the traced image: the next Track's keyframe */
  const float* key_normals;
  const float* frame_depths;   /* the next Track's frame */
  const float* frame_normals;
  const float* pyramid;
  int32_t      key_width, key_height, frame_width, frame_height;
  int32_t      valid;
  int32_t      pad_;
} vk_pyramid_ahead;

/* ref: src/tracer.cpp:41-47,97-100 Tracer::Trace (see above) */
VK_API int vk_trace_ahead_pyramid(const vk_volume* v, const vk_frame* frame, vk_view_bounds* ahead, float* depths, float* colors,
    float* normals, const vk_icp_view* next_frame, float* pyramid, vk_pyramid_ahead* built, void* stream);
/* ref: src/pyramid_tracker.cpp:52-90 PyramidTracker<DepthTracker>::Track, as vk_icp_pyramid_track_frame (see above) */
VK_API int vk_icp_pyramid_track_built(const vk_icp_view* keyframe, const vk_transform* Twm, const vk_icp_view* frame,
    vk_transform* Twc_dev, const vk_transform* Twc_start, int frame_normals_due, vk_pyramid_ahead* built, float* pyramid,
    float* workspace, float* system, int32_t* state_dev, float* update_dev, vk_icp_reduce_fn reduce, void* reduce_user,
    const vk_track_poll* poll, void* stream);

/* ------------------------------------------------------------ colour tracker -- */

/* ref: src/image.cu:10-19,235-247 ColorImage::ConvertTo — intensity = (r+g+b)/3.
 * src: [total*3] floats, dst: [total]. */
VK_API int vk_color_image_convert(int total, const float* src, float* dst, void* stream);

/* ref: src/image.cu:21-99,166-179 Image::GetGradients — 3x3 stencil
 * (1/8, 1/4, 1/8 rows), zero padding outside the image. */
VK_API int vk_image_gradients(int width, int height, const float* src,
    float* gradient_x, float* gradient_y, void* stream);

/* One side of the photometric problem. The keyframe needs depths, normals and
 * intensities; the frame also needs the two gradient images. */
typedef struct vk_color_view {
  const float*  depths;        /* [h*w]   */
  const float*  normals;       /* [h*w*3] */
  const float*  intensities;   /* [h*w]   */
  const float*  gradient_x;    /* [h*w], frame only */
  const float*  gradient_y;    /* [h*w], frame only */
  int32_t       width;
  int32_t       height;
  vk_projection projection;    /* the COLOUR camera's, color_tracker.cu:309-310 */
} vk_color_view;

/* ref: src/color_tracker.cu:43-163,296-344 ColorTracker::ComputeResiduals. One
 * residual per KEYFRAME pixel. Tcm = frame_Tcw * keyframe_Tcw^-1 with
 * X_Tcw = X.depth_to_color * X.depth_to_world^-1 (color_tracker.cu:312-320). */
VK_API int vk_color_tracker_compute_residuals(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_transform* Tcm, float* residuals, void* stream);

/* ref: src/color_tracker.cu:165-204,346-410 ColorTracker::ComputeJacobian;
 * jacobian: [h*w*6] floats, columns 3..5 are 0 when !translation_enabled. */
VK_API int vk_color_tracker_compute_jacobian(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_transform* Tcm, int translation_enabled,
    float* jacobian, void* stream);

/* ref: src/color_tracker.cu:206-343,412-470 ColorTracker::ComputeSystem; same
 * outputs, workspace and fixed-order reduction as vk_icp_compute_system
 * (workspace: vk_icp_workspace_floats(keyframe w, h) floats). `Tcm_dev`:
 * optional DEVICE transform that overrides Tcm. */
VK_API int vk_color_tracker_compute_system(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_transform* Tcm, const vk_transform* Tcm_dev,
    int translation_enabled, float* workspace, float* hessian, float* gradient, void* stream);

/* The frame pose as the device-side loop keeps it. */
typedef struct vk_color_pose {
  vk_transform depth_to_world;  /* frame.depth_to_world_transform, updated in place */
  vk_transform Tcm;             /* derived: what the kernels above consume         */
} vk_color_pose;

/* ref: src/tracker.cpp:124-163 Tracker::ComputeUpdate + src/color_tracker.cpp:
 * 34-96 ColorTracker::ApplyUpdate on the device: solve, M = Tinc *
 * depth_to_world^-1, re-orthonormalise, depth_to_world = (T(t) R)^-1, then
 * Tcm = (frame_Tcd * depth_to_world^-1) * keyframe_Twc for the next iteration.
 * `keyframe_Twc` = (keyframe.depth_to_color * keyframe.depth_to_world^-1)^-1.
 * state_dev / update_dev as in vk_icp_solve_update. */
VK_API int vk_color_tracker_solve_update(const float* hessian, const float* gradient,
    int translation_enabled, const vk_transform* frame_Tcd, const vk_transform* keyframe_Twc,
    vk_color_pose* pose_dev, int32_t* state_dev, float* update_dev, void* stream);

/* ref: src/tracker.cpp:65-76 Tracker::BeginSolve + src/color_tracker.cpp:19-25 ColorTracker::
 * BeginSolve (+ src/light_tracker.cpp:34-41 with `frame_mask`) in ONE launch: the keyframe's and
 * the frame's intensity images (vk_color_image_convert), the frame's gradients
 * (vk_image_gradients), the light tracker's frame mask (vk_light_compute_frame_mask at
 * `depth_threshold`; NULL for the colour tracker), the pose upload into
 * pose_dev->depth_to_world (vk_transform_upload; both NULL to skip) and the reset of
 * state_dev (may be NULL; without a pose upload — a later level of a coarse-to-fine Track — a
 * state that says VK_TRACK_ABORTED is kept, so that the Track fails as a whole). Same bits as the staged calls: the jobs are independent once the
 * gradients take their taps from the colour image, and run side by side. */
VK_API int vk_color_tracker_begin(const vk_frame* keyframe, const vk_frame* frame,
    float* keyframe_intensities, float* frame_intensities, float* gradient_x, float* gradient_y,
    float depth_threshold, float* frame_mask, const vk_transform* pose_host,
    vk_color_pose* pose_dev, int32_t* state_dev, void* stream);

/* ref: src/tracker.cpp:53-63 Tracker::Track for ColorTracker: derive Tcm from
 * pose_dev->depth_to_world, then up to `iterations` Gauss-Newton steps without a host
 * round trip — one launch for the whole loop, as vk_icp_track (three launches per step
 * with `reduce`). Buffers, early exit and VK_TRACK_ABORTED as in vk_icp_track; `workspace`:
 * vk_icp_workspace_floats(keyframe w, h). */
VK_API int vk_color_tracker_track(const vk_color_view* keyframe, const vk_color_view* frame,
    const vk_transform* frame_Tcd, const vk_transform* keyframe_Twc, vk_color_pose* pose_dev,
    int iterations, int translation_enabled, float* workspace, float* system,
    int32_t* state_dev, float* update_dev, vk_icp_reduce_fn reduce, void* reduce_user,
    const vk_track_poll* poll, void* stream);

/* ------------------------------------------------------------- light tracker -- */

/* What LightTracker adds to the colour tracker's inputs (light_tracker.h:52-66):
 * the frame's validity mask, the point light, and the frame's depth->colour
 * extrinsics (its normals are stored in the depth frame). The keyframe's
 * `intensities` are read as albedos. */
typedef struct vk_light_terms {
  const float*  frame_mask;   /* [h*w], vk_light_compute_frame_mask of the frame (light_tracker.cu:19-103 is the same kernel) */
  vk_light      light;
  vk_transform  frame_Tcd;
} vk_light_terms;

/* ref: src/light_tracker.cu:133-330,566-608 LightTracker::ComputeResiduals. Where
 * the mask is set the residual is photometric with a shading model,
 * Ic - albedo * light.GetShading(Xcp, n); elsewhere it falls back to the
 * point-to-plane distance (:283-322). The reference's ComputeResiduals reads
 * frame_mask_ without computing it (:569-577); here the mask is an input. */
VK_API int vk_light_tracker_compute_residuals(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_light_terms* terms, const vk_transform* Tcm,
    float* residuals, void* stream);

/* ref: src/light_tracker.cu:332-371,610-668 LightTracker::ComputeJacobian. The
 * reference evaluates machine-generated expressions (powf / sqrt chains,
 * :233-242); here the same derivative is written in factored form
 * (J_v = grad_p r, J_w = p x grad_p r + n x grad_n r), so values agree with the
 * reference to rounding, not bit for bit — its own finite-difference test
 * (light_tracker_test.cu:454-528, |f - e| < 0.05) is the pin. */
VK_API int vk_light_tracker_compute_jacobian(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_light_terms* terms, const vk_transform* Tcm,
    int translation_enabled, float* jacobian, void* stream);

/* ref: src/light_tracker.cu:373-531,670-732 LightTracker::ComputeSystem; outputs
 * and workspace as vk_color_tracker_compute_system. */
VK_API int vk_light_tracker_compute_system(const vk_color_view* keyframe,
    const vk_color_view* frame, const vk_light_terms* terms, const vk_transform* Tcm,
    const vk_transform* Tcm_dev, int translation_enabled, float* workspace,
    float* hessian, float* gradient, void* stream);

/* ref: src/tracker.cpp:53-63 Tracker::Track for LightTracker. The pose update is
 * ColorTracker's (light_tracker.cpp:50-114 is the same code as
 * color_tracker.cpp:34-96): vk_color_tracker_solve_update, vk_color_pose. */
VK_API int vk_light_tracker_track(const vk_color_view* keyframe, const vk_color_view* frame,
    const vk_light_terms* terms, const vk_transform* keyframe_Twc, vk_color_pose* pose_dev,
    int iterations, int translation_enabled, float* workspace, float* system,
    int32_t* state_dev, float* update_dev, vk_icp_reduce_fn reduce, void* reduce_user,
    const vk_track_poll* poll, void* stream);

/* ---------------------------------------------------------------- detector -- */

/* ref: include/vulcan/detector.h:10-72, src/detector.cu — box detector over a
 * point cloud (nothing upstream instantiates it).
 * `bounds[a]` = {lo, hi}; an axis with lo > hi is unbounded (detector.cu:214-221
 * starts all three at {1,-1}). */
typedef struct vk_detector {
  float   radius;             /* <= 0: no radius test                          */
  float   origin[3];
  float   bounds[3][2];
  int32_t min_inlier_count;   /* fewer survivors => position is NaN            */
  int32_t bounds_use_own_axis;/* 0 = as upstream: the y and z intervals are
                                 tested against point[0] (detector.cu:27-28);
                                 1 = test point[1] / point[2]                  */
} vk_detector;

/* What the detector leaves on the device after a call (one blocking copy reads
 * it all). Sums are fixed-order (4096-point chunks, 256-way strided partials,
 * binary tree, chunks added in order), so every field is reproducible. */
typedef struct vk_detect_state {
  int32_t filtered_count;     /* after the radius / interval test              */
  int32_t inlier_count;       /* after the 1.5-sigma removal                   */
  int32_t detected;           /* inlier_count >= min_inlier_count              */
  int32_t reserved;
  float   center[3];          /* sum|x| / n of the filtered points (Sasum, :137-139) */
  float   limit;              /* 1.5 * sqrt(sum d^2 / n)  (:177-179)           */
  float   position[3];        /* sum|x| / n of the inliers, or NaN             */
  float   squared_error;
} vk_detect_state;

/* bytes of device scratch for a cloud of `count` points (ref: detector.h:66-68
 * points_ / distances_, which this replaces) */
VK_API size_t vk_detect_workspace_bytes(int32_t count);

/* ref: src/detector.cu:152-188 Detector::Filter — interval/radius filter, then
 * removal of points further than 1.5 sigma from the centroid. `inliers`: device
 * float[3*count], receives the survivors in input order (the reference compacts
 * per thread block through an atomic, so its order varies run to run; the set is
 * the same). Fills every field of *state_dev except position / detected. */
VK_API int vk_detect_filter(const vk_detector* detector, const float* points,
    int32_t count, float* inliers, vk_detect_state* state_dev, void* workspace,
    void* stream);

/* ref: src/detector.cu:120-147 Detector::Detect = Filter + BoxDetected +
 * GetValidPosition / GetInvalidPosition; the answer is state_dev->position. */
VK_API int vk_detect(const vk_detector* detector, const float* points,
    int32_t count, float* inliers, vk_detect_state* state_dev, void* workspace,
    void* stream);

/* --------------------------------------------------------------- compaction -- */

/* ref: include/vulcan/util.cuh:52-140 PrefixSum<N> (both overloads) — the stream-compaction
 * primitive behind visible-block, patch and detector compaction. For every element i with
 * counts[i] > 0, offsets[i] is the first of counts[i] private, consecutive slots of a packed
 * output; elements with counts[i] == 0 get -1 (util.cuh:93-94); *total_dev is increased by
 * the sum (it is the reference's `total` argument: zero it to start a new output). The
 * reference leaves the order of the workgroups' ranges to its atomicAdd; here the ranges
 * are in input order (stable). counts, offsets: device int32[count]; workspace: device,
 * vk_compact_workspace_bytes(count). Three launches, no readback. */
VK_API size_t vk_compact_workspace_bytes(int32_t count);
VK_API int vk_compact_offsets(const int32_t* counts, int32_t count, int32_t* offsets,
    int32_t* total_dev, void* workspace, void* stream);

/* --------------------------------------------------------------- extraction -- */

/* ref: include/vulcan/extractor.h:10-136, src/extractor.cu — Extractor::Extract(DeviceMesh&):
 * the triangle mesh of the zero level set. Upstream stops after the vertices
 * (ExtractVertexIndicesKernel / ExtractFacesKernel are empty, extractor.cu:392-430), works one
 * block per launch with blocking copies in between, drops the far faces of every block and
 * has no test; this entry point is the finished extractor (conventions kept, gaps filled:
 * vulcan_amd/csrc/vk_extract.hip). Blocks come from the visible list as upstream
 * (extractor.cu:455-457) or, with `all_allocated`, from the whole table. `interpolate` = 0
 * places a vertex at its edge's midpoint as upstream's active code does (:361), 1 where
 * the linearly interpolated distance is 0.
 * points: device float[3 * point_capacity]; faces: device int32[3 * face_capacity];
 * counts_dev: device int32[4] = {points, faces, cubes skipped because a vertex they need
 * belongs to a block that is not listed, blocks listed}. Counts are the full totals even when
 * a capacity is too small (nothing is written past a capacity). Order: blocks in list order,
 * cubes by z*64 + y*8 + x, vertices by axis, faces in table order — reproducible.
 * workspace: device, vk_extract_workspace_bytes(main, excess) bytes, need not be initialised. Four launches, no readback. */
VK_API size_t vk_extract_workspace_bytes(int32_t main_block_count, int32_t excess_block_count);
VK_API int vk_extract_mesh(const vk_volume* v, int all_allocated, int interpolate, float* points,
    int32_t point_capacity, int32_t* faces, int32_t face_capacity, int32_t* counts_dev,
    void* workspace, void* stream);

/* vk_extract_mesh with a colour and a unit normal per vertex. No upstream counterpart — ref: src/extractor.cu:320-389
 * (ExtractVertexPointsKernel writes a position per cut edge and nothing else) and include/vulcan/mesh.h:10-22 (Mesh and
 * DeviceMesh hold points and faces): upstream has neither attribute, so this comment is the definition;
 * tests/extract_attributes_reference.py states it on the CPU and the device is held to it bit for bit.
 * points, faces, counts_dev, the capacities, the order and the workspace are vk_extract_mesh's, bit for bit; one launch
 * follows its four. colors, normals: device float[3 * point_capacity]; either may be NULL and is then skipped (both
 * NULL: this is vk_extract_mesh). The attributes of vertex i are written iff i < point_capacity.
 * All arithmetic is fp32, one rounding per operation (no contraction); `/` and sqrtf are IEEE-rounded.
 * Vertex i lies on the owned edge `axis` of cube (x, y, z) of a listed block: from lattice point a = (x, y, z) to
 * b = a + e_axis, at t = d(a) / (d(a) - d(b)) when `interpolate`, else 0.5f — the point's own t. A lattice point q
 * (-1 ... 9 per axis, so in one of up to 26 neighbouring blocks, each found by the chain walk of volume.cu:183-190) is
 * KNOWN iff its block is allocated and its voxel's distance_weight != 0 (extractor.cu:202-205).
 * Colour: ca, cb the stored color[3] of a and b, wa, wb their color_weight. Both != 0: c = ca + t * (cb - ca) per
 * channel (sub, mul, add); only one != 0: that voxel's colour; neither: (0, 0, 0).
 * Gradient at a lattice point p (a or b: always known), component k: p + e_k and p - e_k both known:
 * (d(p + e_k) - d(p - e_k)) * 0.5f; only p + e_k known: d(p + e_k) - d(p); only p - e_k known: d(p) - d(p - e_k);
 * neither: 0.0f. Normal: g = ga + t * (gb - ga) per component; n2 = (g.x * g.x + g.y * g.y) + g.z * g.z; n2 > 0:
 * n = g / sqrtf(n2) (three divisions), else (0, 0, 0). It points to the positive-distance side, the side the faces
 * look to. Every vertex is written by its owner cube alone: no atomics, the output does not depend on timing. */
VK_API int vk_extract_mesh_attributes(const vk_volume* v, int all_allocated, int interpolate,
    float* points, float* colors, float* normals, int32_t point_capacity,
    int32_t* faces, int32_t face_capacity, int32_t* counts_dev, void* workspace, void* stream);

/* ------------------------------------------------------------------ release -- */

enum { VK_RELEASE_UNOBSERVED = 1, VK_RELEASE_NO_SURFACE = 2, VK_RELEASE_OUTSIDE_BOX = 4 };

typedef struct vk_release_rule {
  int32_t flags;              /* VK_RELEASE_* or'ed; 0: release nothing, repair only */
  float   min_abs_distance;   /* NO_SURFACE: in units of the stored, normalised distance (-1, 1] */
  int16_t keep_lo[3];         /* OUTSIDE_BOX: block coordinates, inclusive */
  int16_t keep_hi[3];
} vk_release_rule;

/* Give voxel blocks back to the pool, compact the hash table and rebuild the free list — in one call, nothing read
 * back, the result independent of timing. No upstream counterpart: ref: src/volume.cu:304-368 (HandleAllocationRequests)
 * pops pool slots and bumps the excess pointer and never returns a slot, unlinks an entry or lowers the pointer; once
 * the excess list is full it leaks one pool slot per refused request (:337-356) and, once the pool is empty, links
 * excess entries it never writes ("ghosts", :344). The definition is this comment; tests/release_reference.py states it
 * on the CPU and the device is held to it bit for bit.
 * PRECONDITION (the caller's duty here; the class layers enforce it): the volume is between SetView calls —
 * allocation_types all NONE, no frame announced (vk_requests_ahead) and its SetView outstanding.
 * Released: a block (an entry with data >= 0 that is reachable from a main bucket along `next`) for which an enabled
 * rule holds — UNOBSERVED: all 512 voxels have distance_weight == 0; NO_SURFACE: a voxel has distance_weight != 0 and
 * no such voxel has fabsf(distance) < min_abs_distance; OUTSIDE_BOX: origin[a] < keep_lo[a] or origin[a] > keep_hi[a]
 * for some a. Only stored values are compared, nothing is computed.
 * Afterwards: (chains) for every main bucket b, ascending, the entries of its chain — entry b included — that hold a
 * block which stays, in chain order: the first at entry b, the others at consecutive excess entries starting at
 * main + sum over b' < b of max(survivors(b') - 1, 0), linked in that order, the last `next` -1; every other entry is
 * HashEntry() (origin 0, pad 0, data -1, next -1); VK_CTR_EXCESS_PTR = main + survivors in excess entries.
 * (visibility) a survivor's block_visibility byte moves with it, every other byte is VK_VISIBILITY_FALSE,
 * VK_CTR_VISIBLE = 0, VK_CTR_BANDED = -1: the caller's next SetView rebuilds the visible list. (pool)
 * free_voxel_blocks[k] = the k-th pool slot, ascending, that no survivor references, -1 behind them, VK_CTR_VOXEL_PTR =
 * their number - 1 — slots upstream's allocator leaked come back; on a fresh volume this is Initialize's list.
 * (voxels) the 512 voxels of every released block are Voxel::Empty() (distance 1, colour 0, weights 0: what the
 * allocator assumes of a fresh slot); no other voxel byte changes. counts_dev: device int32[4] = {blocks released,
 * blocks kept, excess entries in use, free slots}. VK_CTR_DROPPED and the other public counters are untouched.
 * With flags == 0 the call is a pure repair: it removes ghosts, makes the excess entries dense and rebuilds the free
 * list. Anything prepared ahead for the volume is VOID after the call and must be invalidated by the caller: the
 * vk_view_bounds records (valid = 0), a vk_light_prep (valid = 0), and no vk_requests_ahead record may be valid.
 * v->voxels 16-byte aligned. workspace: device, vk_volume_release_workspace_bytes(main, excess) bytes (0 for sizes that
 * are not a volume's), need not be initialised. Thirteen short launches on `stream` (the two ordered scans are vk_compact_offsets'); only released blocks' voxels are written
 * and only allocated blocks' voxels are read (none when OUTSIDE_BOX is the only rule). */
VK_API size_t vk_volume_release_workspace_bytes(int32_t main_block_count, int32_t excess_block_count);
VK_API int vk_volume_release_blocks(const vk_volume* v, const vk_release_rule* rule,
    int32_t* counts_dev /* [4] */, void* workspace, void* stream);

/* -------------------------------------------------------------------- merge -- */

enum { VK_MERGE_SKIP_UNOBSERVED = 1, VK_MERGE_CONTINUE = 2 };

typedef struct vk_merge_params {
  int32_t flags;                /* VK_MERGE_* or'ed */
  int32_t max_rounds;           /* >= 1 */
  float   max_distance_weight;  /* 1 .. 32767 */
  float   max_color_weight;     /* 1 .. 32767 */
} vk_merge_params;

/* Fuse volume `src` into volume `dst`: allocate in dst the blocks of src it lacks, then continue every voxel's running
 * average with the source's value and weight — in one call, nothing read back, the result independent of timing. No
 * upstream counterpart (its Volume is a process-wide singleton, src/volume.cu:17-21); ref: src/volume.cu:304-368 for the
 * allocation (HandleAllocationRequests, reused as it is), src/depth_integrator.cu:55-59 and
 * src/color_integrator.cu:109-118 for the running average (there the new sample has weight 1, here the source voxel's).
 * The definition is this comment; tests/merge_reference.py states it on the CPU and the device is held to it bit for bit.
 * PRECONDITIONS (the caller's duty; the class layers enforce them): both volumes are between SetView calls —
 * allocation_types all NONE, no frame announced (vk_requests_ahead); src is only read. Checked on the host, VK_ERR_ARGUMENT
 * with no device touched: a null argument or buffer, dst->voxels == src->voxels, voxel_length or truncation_length not
 * bitwise equal, a voxel pool not 16-byte aligned, an unknown flag, max_rounds < 1, a cap outside 1 .. 32767.
 * main_block_count and excess_block_count may differ between the two.
 * (source blocks) an entry of src that is reachable from a main bucket along `next` and has data >= 0. With
 * SKIP_UNOBSERVED a block all of whose 512 voxels have distance_weight == 0 and color_weight == 0 is ignored: neither
 * requested nor fused (one extra read of the allocated part of the source pool).
 * (presence) a block is present in dst when the chain of its bucket hash(origin) % dst->main_block_count holds an entry
 * with data >= 0 and that origin. The empty main entry does not stand in for block (0,0,0).
 * (allocation) at most max_rounds rounds. In a round every considered block that is absent posts one request in its dst
 * bucket: VK_ALLOC_MAIN if that main entry has data == -1, else VK_ALLOC_EXCESS; the bucket goes to the largest key
 * (type << 48 | z << 32 | y << 16 | x, the coordinates as uint16: what SetView's request pass writes, with pad = type);
 * a MAIN request sets the bucket's block_visibility to TRUE (volume.cu:193-200). Then one handle pass, exactly
 * vk_volume_handle_allocation_requests (exhaustion included: leaked slots, never-written excess entries). The rounds end
 * with a round that posts nothing — it runs no handle pass — and after a round whose handle pass raised VK_CTR_DROPPED.
 * (fusion) for every considered block present in dst after the rounds, voxel i of the source block into voxel i of the
 * dst block, fp32, one rounding per operation, no contraction, IEEE division. If s.distance_weight != 0: wd =
 * (float)d.distance_weight, ws = (float)s.distance_weight, sum = wd + ws; d.distance = wd == 0 ? s.distance :
 * (wd * d.distance + ws * s.distance) / sum; d.distance_weight = (int16_t)fminf(max_distance_weight, sum). If
 * s.color_weight != 0: the same per colour channel with the colour weights and max_color_weight. A field whose source
 * weight is 0 keeps its bytes. Blocks still absent are left out. Each call fuses what it finds present: the same pair
 * merged twice counts the source twice.
 * (CONTINUE) `workspace` is the one the previous call for this pair left, neither volume's table has been changed
 * since by anything but that call: the blocks that call left out are the considered blocks of this one (SKIP_UNOBSERVED
 * has no further effect), what it fused is not fused again. A merge split into calls this way runs the same rounds and
 * leaves the same state as one call with the rounds of all of them.
 * (afterwards) VK_CTR_VISIBLE = 0, VK_CTR_BANDED = -1: the caller's next SetView rebuilds the visible list; VK_CTR_REQUESTS
 * is the last handle pass's; anything prepared ahead for dst is VOID as after vk_volume_release_blocks. counts_dev:
 * device int32[6] = {source blocks considered, blocks fused, blocks allocated by the call, source blocks left out,
 * rounds that posted a request, source blocks skipped as unobserved}. workspace: device,
 * vk_volume_merge_workspace_bytes(src main, src excess) bytes (0 for sizes that are not a volume's), need not be
 * initialised: the one thing a workspace carries from call to call is what a CONTINUE call takes over. 5 + 4 * max_rounds
 * short launches on `stream` and one pass of one wave per source block over the two voxel pools. Moving a replica
 * between devices is the caller's: both volumes' buffers are on the stream's device (vk_volume_pack below makes the replica
 * two compact arrays to copy, and vk_volume_merge_packed merges them). */
VK_API size_t vk_volume_merge_workspace_bytes(int32_t src_main, int32_t src_excess);
VK_API int vk_volume_merge(const vk_volume* dst, const vk_volume* src, const vk_merge_params* p,
    int32_t* counts_dev /* [6] */, void* workspace, void* stream);

/* ----------------------------------------------------------- merge through a pose -- */

typedef struct vk_merge_pose_params {
  vk_merge_params merge;        /* flags (SKIP_UNOBSERVED, CONTINUE), max_rounds, the two caps: as vk_volume_merge */
  vk_transform    pose;         /* T_dst_src: x_dst = m * x_src, metres; m and inv are both used as given */
} vk_merge_pose_params;

/* Fuse volume `src` into volume `dst` through a rigid pose: the two volumes need not share a world frame or a voxel
 * lattice, every dst voxel takes a trilinear sample of src at its own centre carried back into src's frame. What
 * vk_volume_merge leaves out ("resampling"). No upstream counterpart (its Volume is a process-wide singleton,
 * src/volume.cu:17-21); ref: src/volume.cu:304-368 for the allocation, src/depth_integrator.cu:55-59 and
 * src/color_integrator.cu:109-118 for the running average, oracle_integrate.c:12-15 for a voxel's centre (there in metres).
 * The definition is this comment;
 * tests/merge_pose_reference.py states it on the CPU and the device is held to it bit for bit. All arithmetic is fp32,
 * one rounding per operation, no contraction, IEEE division.
 * PRECONDITIONS and host checks: vk_volume_merge's, and every one of the 24 entries of rows 0-2 of pose.m and pose.inv is
 * finite, else VK_ERR_ARGUMENT with no device touched. That m is rigid and inv its inverse is the caller's duty (the
 * class layers build both from one Transform); with anything else the call stays inside its buffers and ends, and the
 * counts of blocks may count a block more than once.
 * (coordinates) voxel units. Voxel (x,y,z) of block B has centre c_a = (float)(8 B_a + i_a) + 0.5f; tm_a = m[12+a] /
 * voxel_length, ti_a = inv[12+a] / voxel_length; fwd(c)_a = ((m[a] c_0 + m[4+a] c_1) + m[8+a] c_2) + tm_a, back(c) the
 * same with inv and ti. Stored distances are in truncation lengths, which the volumes share: values are not rescaled.
 * (source blocks) vk_volume_merge's, SKIP_UNOBSERVED included.
 * (candidates) for a considered source block with origin o: the corners (float)(8 o_a + 8 s_a), s in {0,1}^3, through
 * fwd; lo_a = (int)floorf(min_a * 0.125f), hi_a = (int)floorf(max_a * 0.125f) (fminf / fmaxf; the conversion saturates,
 * NaN gives 0; both are then clamped to +-40000, which changes no block inside the int16 range), hi_a capped at lo_a + 2.
 * A block B in [lo, hi]^3 with every coordinate in the int16 range is a candidate of o if and only if it has a voxel
 * whose cell = floorf(back(c)) has 8 o_a <= cell_a <= 8 o_a + 7 on all three axes. The candidates of the call are the
 * union over the considered source blocks, each dst block once.
 * (allocation) vk_volume_merge's rounds with the candidates in the place of the source blocks: presence by the chain
 * walk, one request per bucket and round, MAIN or EXCESS, the largest key wins, a MAIN request sets visibility TRUE, one
 * vk_volume_handle_allocation_requests per round, the same two ends of the rounds.
 * (fusion) for every candidate present after the rounds, every voxel: p = back(c), g_a = p_a - 0.5f, b_a = floorf(g_a),
 * f_a = g_a - b_a. The lattice point b + s, s in {0,1}^3, is USED iff for every axis s_a == 0 or f_a != 0. Lattice point
 * n is voxel (n mod 8) — index z*64 + y*8 + x — of source block floor(n / 8), found by the chain walk (absent when a
 * coordinate leaves the int16 range). A distance sample exists iff every USED point's block is present and its
 * distance_weight != 0; its value is the lerp a + f * (b - a) (sub, mul, add) along x, then y, then z, an axis with
 * f == 0 taking its base value; its weight ws is (float) of the smallest distance_weight over the USED points. A colour
 * sample likewise, per channel, with color_weight. Each sample continues the voxel's running average as vk_volume_merge
 * does with a source voxel of that value and weight; a field without a sample keeps its bytes. A candidate that receives
 * no sample at all stays allocated and Voxel::Empty(): vk_volume_release_blocks(VK_RELEASE_UNOBSERVED) gives such blocks
 * back. One wave writes a dst block; no atomic touches a voxel.
 * (CONTINUE) `workspace` is the previous call's for this pair and pose, no table changed since but by that call: the call
 * considers the same source blocks and the same candidates, passes over the candidates already fused, and with the
 * earlier calls runs the rounds and leaves the state of one call with as many rounds.
 * (afterwards) as vk_volume_merge. counts_dev: device int32[8] = {source blocks considered, candidate dst blocks (of a
 * CONTINUE call: those not fused before), candidates fused, blocks allocated by the call, candidates left out, rounds
 * that posted, source blocks skipped as unobserved (0 in a CONTINUE call), voxels that took a distance sample}.
 * workspace: device, vk_volume_merge_posed_workspace_bytes(...) bytes (0 for sizes that are not a volume's), need not be
 * initialised (a CONTINUE call's excepted, as vk_volume_merge's). */
VK_API size_t vk_volume_merge_posed_workspace_bytes(int32_t src_main, int32_t src_excess, int32_t dst_main, int32_t dst_excess);
VK_API int vk_volume_merge_posed(const vk_volume* dst, const vk_volume* src, const vk_merge_pose_params* p,
    int32_t* counts_dev /* [8] */, void* workspace, void* stream);

/* ------------------------------------------- merge through a pose and a change of scale -- */

typedef struct vk_merge_resample_params {
  vk_merge_params merge;      /* flags, max_rounds, the two caps: as vk_volume_merge */
  vk_transform    pose;       /* T_dst_src, metres; m and inv both used as given */
  int32_t         supersample;/* n in 1..4: n^3 sample points per dst voxel */
  int32_t         reserved;   /* 0 */
} vk_merge_resample_params;

/* Fuse volume `src` into volume `dst` through a rigid pose when the two differ in voxel length, in truncation length or
 * in both: vk_volume_merge_posed with a change of scale. A coarser destination takes the mean of n^3 sample points per
 * voxel (a box filter against aliasing), and the stored distances, which are in truncation lengths, are carried into the
 * destination's. No upstream counterpart; ref: as vk_volume_merge_posed, and src/depth_integrator.cu for the band a
 * stored distance lies in ((-1, 1]: the integrator never writes behind the band). The definition is this comment: it is
 * vk_volume_merge_posed's with the changes below, and at bitwise equal lengths with supersample == 1 it is that
 * definition word for word. tests/merge_resample_reference.py states it on the CPU and the device is held to it bit for
 * bit. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division.
 * PRECONDITIONS and host checks: vk_volume_merge_posed's, except that the lengths may differ. r_fwd = src->voxel_length /
 * dst->voxel_length and r_back = dst->voxel_length / src->voxel_length (one division each) both lie in [0.25, 4];
 * k = src->truncation_length / dst->truncation_length is finite and > 0; supersample is in 1..4; reserved == 0. Anything
 * else is VK_ERR_ARGUMENT with no device touched.
 * (coordinates) each volume's own voxel units. fwd(c)_a = ((fm[a][0] c_0 + fm[a][1] c_1) + fm[a][2] c_2) + tm_a with
 * fm[a][j] = m[4j+a] * r_fwd and tm_a = m[12+a] / dst->voxel_length; back(c) the same with inv, r_back and
 * inv[12+a] / src->voxel_length. (x * 1.0f == x: at r == 1.0f these are vk_volume_merge_posed's.)
 * (sample points) a dst voxel with centre c has n^3 points p = c + (o_jx, o_jy, o_jz), jx fastest, then jy, then jz,
 * o_j = (float)(2j+1) / (float)(2n) - 0.5f; n == 1 gives o == 0.0f and p == c bitwise.
 * (source blocks) vk_volume_merge's, SKIP_UNOBSERVED included.
 * (candidates) the box [lo, hi]^3 of a considered source block from its eight corners through fwd as
 * vk_volume_merge_posed defines it, hi_a capped at lo_a + K - 1 with K = min(8, (int)(r_fwd * 1.7320508f) + 2): a block
 * of 8 r_fwd voxels spans no more along an axis than its diagonal (3 at ratio 1). A block B of the box with every
 * coordinate in the int16 range is a candidate of o iff one of its voxels has a sample point p whose cell =
 * floorf(back(p)) has 8 o_a <= cell_a <= 8 o_a + 7 on all three axes.
 * (allocation) vk_volume_merge's rounds with the candidates in the place of the source blocks, unchanged.
 * (a sub-sample) vk_volume_merge_posed's trilinear sample at back(p) for a sample point p: g_a = back(p)_a - 0.5f, the
 * USED lattice points, the lerps along x, then y, then z, the weight the smallest over the USED points; distance and
 * colour apart. When k != 1.0f (bitwise) the distance sub-sample goes on: for k < 1 it does not exist if the stored
 * distance of a USED point is >= 1.0f (a saturated value says "at least one source truncation length away", which
 * cannot be said in the destination's units); else d' = k * d; d' >= 1 becomes 1.0f; d' <= -1 makes the sub-sample not
 * exist (nothing is stored behind the band). Colour is not rescaled.
 * (a voxel's sample) per field it exists iff more than half of the n^3 sub-samples exist, 2 * count > n^3; its value is
 * the sum of those sub-samples in point order — the first, then + the next, ... — divided by (float)count, per channel
 * for colour; its weight is the smallest of their weights. It continues the voxel's running average as
 * vk_volume_merge does with a source voxel of that value and weight, the caps included; a field without a sample keeps
 * its bytes. One wave writes a dst block; no atomic touches a voxel.
 * (CONTINUE), (afterwards) and the eight counts: vk_volume_merge_posed's; counts[7] counts the voxels that took a
 * distance sample. A CONTINUE call takes the previous call's workspace for this pair, pose and supersample.
 * workspace: device, vk_volume_merge_resampled_workspace_bytes(..., K) bytes with the K above (0 for sizes that are not a
 * volume's or a K outside 2..8), need not be initialised (a CONTINUE call's excepted). */
VK_API size_t vk_volume_merge_resampled_workspace_bytes(int32_t src_main, int32_t src_excess,
    int32_t dst_main, int32_t dst_excess, int32_t box_blocks_per_axis);
VK_API int vk_volume_merge_resampled(const vk_volume* dst, const vk_volume* src, const vk_merge_resample_params* p,
    int32_t* counts_dev /* [8] */, void* workspace, void* stream);

/* --------------------------------------------------------------- pack the blocks -- */

typedef struct vk_block_pack {
  int32_t   capacity;   /* blocks the two arrays can hold */
  int32_t   pad;
  int16_t*  origins;    /* device [4 * capacity], 8-byte aligned: block x, y, z, 0 */
  vk_voxel* voxels;     /* device [512 * capacity], 16-byte aligned; NULL: count only */
} vk_block_pack;

enum { VK_PACK_SKIP_UNOBSERVED = 1, VK_PACK_BOX = 2 };

typedef struct vk_pack_rule {
  int32_t flags;        /* VK_PACK_* or'ed */
  int16_t lo[3], hi[3]; /* BOX: block coordinates, inclusive */
} vk_pack_rule;

/* The blocks of a volume, compact and in a defined order: what a caller writes to a file, hands to another device or
 * process, and merges there (the receiving side follows below) — at the cost of the blocks that exist, not of the pool. No
 * upstream counterpart (its Volume is a process-wide singleton that never leaves its buffers, ref: src/volume.cu:17-21;
 * the chain walk is that of src/volume.cu:183-190). The definition is this comment; tests/pack_reference.py states it on
 * the CPU and the device is held to it byte for byte.
 * The call only READS the volume: it is allowed while a frame is announced (vk_requests_ahead), and no counter changes.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v, pack, counts_dev or workspace null, a volume that vk_volume_merge
 * would refuse for a null buffer, its sizes or its alignment, rule->flags with an unknown bit, BOX with lo[a] > hi[a] on an
 * axis, capacity < 0, and with voxels != NULL: origins null or not 8-byte aligned, voxels not 16-byte aligned. rule == NULL:
 * every block.
 * (source blocks) vk_volume_merge's: an entry that is reachable from a main bucket along `next` and has data >= 0.
 * (selection) a source block is SELECTED unless BOX is set and origin[a] < lo[a] or origin[a] > hi[a] for some a, or — of
 * the blocks the box leaves — SKIP_UNOBSERVED is set and all 512 voxels have distance_weight == 0 and color_weight == 0
 * (vk_volume_merge's test; one extra read of those blocks). Only stored values are compared.
 * (order) the selected blocks in ascending order of their table entry index: main entries first, then excess entries. The
 * positions come from an ordered scan (vk_compact_offsets); no atomic decides one, the pack is the same every time.
 * (the pack) with written = min(selected, capacity): block k < written is that entry's origin in origins[4k .. 4k+2],
 * origins[4k+3] = 0, and the 10 240 bytes of pool slot `data` in voxels[512k ..], byte for byte. Nothing is written at or
 * behind block `written`. With voxels == NULL nothing is written at all and written = 0: the call only counts, so that
 * the caller can size the pack. Origins within a pack are distinct.
 * counts_dev: device int32[4] = {source blocks, selected, written, blocks the box left that were skipped as unobserved}.
 * workspace: device, vk_volume_pack_workspace_bytes(main, excess) bytes (0 for sizes that are not a volume's), need not be
 * initialised. Six short launches on `stream` (seven with SKIP_UNOBSERVED) and, with voxels, one pass of one wave per
 * packed block: ten 16-byte loads and stores per lane. Nothing is read back. Moving a pack to another device is two plain
 * copies, of origins and of voxels. */
VK_API size_t vk_volume_pack_workspace_bytes(int32_t main_block_count, int32_t excess_block_count);
VK_API int vk_volume_pack(const vk_volume* v, const vk_pack_rule* rule /* NULL: every block */,
    const vk_block_pack* pack, int32_t* counts_dev /* [4] */, void* workspace, void* stream);

/* vk_volume_merge with "the considered source blocks" replaced by blocks 0 .. block_count-1 of a pack; no new arithmetic
 * (ref: src/volume.cu:304-368 for the allocation, src/depth_integrator.cu:55-59 and src/color_integrator.cu:109-118 for
 * the running average, as at vk_volume_merge, whose comment is the definition; tests/pack_reference.py states the
 * replacement on the CPU). Presence, the allocation rounds, the handle pass, the fusion arithmetic and the caps are
 * merge's own — one source compiles both — and so are SKIP_UNOBSERVED (classified from the packed voxels), CONTINUE, the
 * six counts and "afterwards". In one sentence: for a pack made without a rule from a volume src, with block_count =
 * written = selected, the call leaves dst and counts_dev bit for bit as vk_volume_merge(dst, src, p) leaves them — entries,
 * visibility, free list, voxels and counters.
 * PRECONDITIONS: vk_volume_merge's for dst (between SetView calls, no frame announced: the class layers enforce it). The
 * pack is only read. The origins of blocks 0 .. block_count-1 are DISTINCT and their fourth component is 0: the caller's
 * duty — vk_volume_pack guarantees it, the file loaders of the class layers check it on the host. With duplicates the call
 * stays inside its buffers and ends; which duplicate's voxels arrive in dst, or which mixture, is undefined.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): dst, pack, p, counts_dev or workspace null, origins or voxels null,
 * origins not 8-byte or voxels not 16-byte aligned, pack->voxels == dst->voxels, a dst or a p that vk_volume_merge would
 * refuse, voxel_length or truncation_length not bitwise equal to dst's, block_count outside 0 .. capacity.
 * block_count == 0: VK_OK after the checks, six zero counts, "afterwards" as merge leaves it for a source without blocks.
 * workspace: device, vk_volume_merge_packed_workspace_bytes(block_count) bytes (0 for a negative count), need not be
 * initialised — what a CONTINUE call takes over excepted, as for vk_volume_merge. 4 + 4 * max_rounds short launches on
 * `stream` and one pass of one wave per packed block. */
VK_API size_t vk_volume_merge_packed_workspace_bytes(int32_t block_count);
VK_API int vk_volume_merge_packed(const vk_volume* dst, const vk_block_pack* pack, int32_t block_count,
    float voxel_length, float truncation_length, const vk_merge_params* p,
    int32_t* counts_dev /* [6], vk_volume_merge's */, void* workspace, void* stream);

/* ------------------------------------------------------- register volume to volume -- */

typedef struct vk_register_params {
  int32_t flags;             /* 0; reserved, anything else VK_ERR_ARGUMENT */
  int32_t iterations;        /* 1 .. 64 */
  float   max_abs_distance;  /* band, in truncation lengths: 0 < band <= 1 */
  int32_t pad;
} vk_register_params;

#define VK_REGISTER_NO_OVERLAP 2   /* state_dev[1]: a step found no residual */

/* Refine the rigid pose T_dst_src between two volumes — the pose vk_volume_merge_posed takes — by Gauss-Newton on the two
 * TSDFs themselves: every source voxel near the surface is carried into dst, dst's field is sampled there, and the pose
 * moves so that the sample equals the voxel's own distance. It REFINES a guess that already brings the two surfaces
 * within roughly a truncation length of each other where they overlap; it searches nothing, and a periodic scene locks
 * on to the nearest period. No upstream counterpart; ref: src/tracker.cpp:124-163 for the loop and its end,
 * src/color_tracker.cpp:45-95 for the step. The definition is this comment; tests/register_reference.py states it on the
 * CPU. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division.
 * ACCESS: both volumes are only read; dst == src is allowed; the table sizes may differ.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): a null argument or buffer (update_dev alone may be null), a volume
 * that vk_volume_merge would refuse for its sizes or alignment, voxel_length or truncation_length not bitwise equal
 * between the two, flags != 0, iterations outside 1 .. 64, the band not in (0, 1] (a NaN included).
 * The pose is on the device (vk_transform_upload seeds it). m is used as given; the solve rewrites m and inv together.
 * (coordinates) vk_volume_merge_posed's: voxel i = z*64 + y*8 + x of block B has centre c_a = (float)(8 B_a + i_a) + 0.5f;
 * tm_a = m[12+a] / voxel_length; fwd(c)_a = ((m[a] c_0 + m[4+a] c_1) + m[8+a] c_2) + tm_a.
 * (source voxels) the source blocks are vk_volume_merge's: reachable from a main bucket along `next`, data >= 0. A source
 * voxel s is IN BAND iff s.distance_weight != 0 and fabsf(s.distance) < band.
 * (sample) p = fwd(c), g_a = p_a - 0.5f, b_a = floorf(g_a), f_a = g_a - b_a. The eight lattice points b + k, k in {0,1}^3,
 * are voxels of dst found by the chain walk; a point is absent when a block coordinate leaves the int16 range. The sample
 * exists iff all eight are present with distance_weight != 0 (the gradient needs both ends of every axis: there is no
 * "used points" rule here). v[k], k = kx + 2 ky + 4 kz, are their distances; lerp(t,a,b) = a + t*(b - a) (sub, mul, add).
 *   x00 = lerp(fx,v0,v1), x10 = lerp(fx,v2,v3), x01 = lerp(fx,v4,v5), x11 = lerp(fx,v6,v7)
 *   y0 = lerp(fy,x00,x10), y1 = lerp(fy,x01,x11), D = lerp(fz,y0,y1)
 *   gz = y1 - y0, gy = lerp(fz, x10 - x00, x11 - x01),
 *   gx = lerp(fz, lerp(fy, v1 - v0, v3 - v2), lerp(fy, v5 - v4, v7 - v6))       (truncation lengths per voxel)
 * (residual) exists iff the voxel is in band, the sample exists and fabsf(D) < band. Then r = D - s.distance, weight 1,
 *   J0 = p1*gz - p2*gy, J1 = p2*gx - p0*gz, J2 = p0*gy - p1*gx      (x cross gradient in metres: the voxel length cancels)
 *   J3 = gx*iv, J4 = gy*iv, J5 = gz*iv, iv = 1.0f / voxel_length computed once
 * — the depth tracker's form (X x n, n); the unknown is a twist applied on the left of T_dst_src, in dst's frame.
 * (system) system[0..21) is the packed lower triangle of sum J J^T, row-major as vk_icp_compute_system's, system[36..42)
 * is sum J r, system[42] is sum r^2, the rest 0. The reduction has one fixed order that depends on the source's table
 * sizes alone: the same inputs give the same bits every call. counts = {source blocks considered, source voxels in band,
 * residuals, 0}.
 * (step) the colour trackers' step: update = -H^-1 g by the library's LDL^T (the zero update for a rank-deficient system),
 * M = Tinc(update) * m with the proper skew matrix, pose <- rigid_from(M), m and inv together; an update of six zeros
 * leaves the pose's bytes alone (no re-orthonormalisation, no change of a zero's sign).
 * state_dev = {steps run, code}, zeroed by the caller. code 0: running; 1: converged, |update| < 1e-6 (tracker.cpp:162; that
 * step's pose is written like any other's); VK_REGISTER_NO_OVERLAP: a step whose residual count is 0 — it counts as a step,
 * leaves the pose's bytes alone and writes a zero update.
 * vk_volume_register enqueues `iterations` steps on `stream`, launch per stage (a residual pass, the sum, a one-wave solve),
 * with no host round trip and nothing read back; nothing in it waits inside a launch, so it cannot hang a device. The
 * source blocks are listed once per call. A stage that finds state_dev[1] != 0 returns at once, so system_dev and
 * counts_dev hold the last evaluated step's values, those of the pose BEFORE that step's update.
 * vk_volume_register_system: one evaluation at the pose. vk_volume_register_terms: for source pool slot q and voxel i,
 * valid[q*512+i], residuals[q*512+i] and jacobians[(q*512+i)*6 ..], zeros where no residual exists; the three buffers
 * hold (src main + excess) * 512 voxels.
 * workspace: device, vk_volume_register_workspace_bytes(src main, src excess) bytes (0 for sizes that are not a volume's),
 * need not be initialised. */
VK_API size_t vk_volume_register_workspace_bytes(int32_t src_main, int32_t src_excess);
VK_API int vk_volume_register_terms(const vk_volume* dst, const vk_volume* src, const vk_transform* pose_dev,
    const vk_register_params* p, float* residuals, float* jacobians, uint8_t* valid, void* workspace, void* stream);
VK_API int vk_volume_register_system(const vk_volume* dst, const vk_volume* src, const vk_transform* pose_dev,
    const vk_register_params* p, float* system_dev, int32_t* counts_dev, void* workspace, void* stream);
VK_API int vk_volume_register(const vk_volume* dst, const vk_volume* src, vk_transform* pose_dev /* in: start, out: result */,
    const vk_register_params* p, float* system_dev /* [48] */, int32_t* state_dev /* [2] */, int32_t* counts_dev /* [4] */,
    float* update_dev /* optional [6] */, void* workspace, void* stream);

/* ------------------------------------------------------------------ sample -- */

enum { VK_SAMPLE_VOXEL_UNITS = 1, VK_SAMPLE_DISTANCE_ONLY = 2 };

typedef struct vk_sample_params {
  int32_t flags;             /* VK_SAMPLE_*; an unknown bit is VK_ERR_ARGUMENT */
  int32_t pad;
} vk_sample_params;

/* The volume's field at arbitrary points: for each of `count` points the trilinear sample of the stored voxels — signed
 * distance, colour and the two weights, as a vk_voxel — and the gradient of the distance. What a planner, a collision
 * check or a tool that rates a reconstruction asks of a TSDF map. No upstream counterpart (the reference samples its
 * volume only along camera rays); ref: src/tracer.cu:238-299 for the trilinear sample of a ray, src/volume.cu:168-191 for
 * the chain walk. The definition is this comment; tests/sample_reference.py states it on the CPU and the device is held
 * to it bit for bit. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division.
 * ACCESS: the volume is only read. One launch on `stream`, nothing read back, no atomic and no wait on another workgroup:
 * it cannot hang a device.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v or p null, a volume that vk_volume_merge would refuse for its sizes
 * or alignment, a flag other than the two, count < 0, points null with count > 0, samples and gradients both null,
 * gradients not 16-byte aligned. count == 0 returns 0 and launches nothing.
 * (coordinates) point i is x = points[3i .. 3i+2], in metres, in the frame that pose_dev carries into the volume's.
 * q_a = x_a / voxel_length; with VK_SAMPLE_VOXEL_UNITS q = x and nothing is divided. With pose_dev == NULL p = q, else
 * p = fwd(q) as vk_volume_merge_posed defines fwd: fwd(q)_a = ((m[a] q_0 + m[4+a] q_1) + m[8+a] q_2) + tm_a with
 * tm_a = m[12+a] / voxel_length; inv is not read. The pose is read on the device (vk_transform_upload seeds one; a
 * tracker's pose that never left the device can be handed in). A point with a non-finite component of p has no sample of
 * any kind.
 * (lattice) g_a = p_a - 0.5f, b_a = floorf(g_a), f_a = g_a - b_a; b is converted to int (saturating) and clamped to
 * +-2^30. The lattice point n = b + s, s in {0,1}^3, is voxel (n mod 8) — index z*64 + y*8 + x — of block floor(n / 8),
 * found by the chain walk; a point is absent when a block coordinate leaves the int16 range.
 * (the sample, a vk_voxel) vk_volume_merge_posed's, word for word: b + s is USED iff for every axis s_a == 0 or
 * f_a != 0; a distance sample exists iff every USED point is present with distance_weight != 0; its value is the lerp
 * a + f * (b - a) (sub, mul, add) along x, then y, then z, an axis with f == 0 taking its base value; its
 * distance_weight is the smallest distance_weight over the USED points. The colour likewise, per channel, with
 * color_weight. A field without a sample is Voxel::Empty()'s: distance 1.0f (never 0: a caller who ignores the weight
 * reads "far from any surface"), colour 0, weight 0. Distances are in truncation lengths, as stored. With
 * VK_SAMPLE_DISTANCE_ONLY the colour fields are 0 and no colour byte of the pool is read.
 * (the gradient) gradients[4i .. 4i+3] = {gx, gy, gz, 1.0f} with vk_volume_register's gx, gy, gz over the eight
 * distances v[k], k = kx + 2 ky + 4 kz, in truncation lengths per voxel, in the volume's frame. It exists iff all eight
 * points are present with distance_weight != 0 (no USED rule: the gradient needs both ends of every axis); otherwise the
 * four floats are 0. The fourth float is the validity: a zero gradient in free space is a real value.
 * (writes) samples[i] and gradients[4i ..] for i < count only, each by its own lane; a null output is not written. */
VK_API int vk_volume_sample(const vk_volume* v, const float* points /* device [3*count] */, int32_t count,
    const vk_transform* pose_dev /* optional, device: T_volume_points */, const vk_sample_params* p,
    vk_voxel* samples /* optional, device [count] */, float* gradients /* optional, device [4*count] */, void* stream);

/* --------------------------------------------------------------- cast rays -- */

enum { VK_CAST_VOXEL_UNITS = 1, VK_CAST_DISTANCE_ONLY = 2 };
enum { VK_RAY_MISS = 0, VK_RAY_HIT = 1, VK_RAY_STEPS = 2, VK_RAY_INVALID = 3 };

typedef struct vk_cast_params {
  int32_t flags;             /* VK_CAST_*; an unknown bit is VK_ERR_ARGUMENT */
  int32_t max_steps;         /* 1 .. 65536: the march of a ray takes at most this many steps */
  float t_min;               /* 0 <= t_min < t_max, both finite: the stretch of the ray that is searched, in metres */
  float t_max;               /*   along the normalised direction (in voxels with VK_CAST_VOXEL_UNITS) */
} vk_cast_params;

/* What each of `count` arbitrary rays through the volume hits first, and how far away: a line of sight or a collision
 * check for a planner, a simulated LiDAR or fisheye sensor, picking in a viewer, a next-best-view score, a camera model
 * vk_trace does not have. No upstream counterpart (the reference casts only the pixel rays of one pinhole camera, and
 * vk_trace needs that camera's frame, visible-block list and patch bounds); ref: src/tracer.cu:317-451 for the march rule,
 * which this is in voxel units, src/volume.cu:168-191 for the chain walk. The definition is this comment;
 * tests/cast_reference.py states it on the CPU and the device is held to it bit for bit. All arithmetic is fp32, one
 * rounding per operation, no contraction, IEEE division and a correctly rounded square root.
 * ACCESS: the volume is only read. One launch on `stream`, nothing read back, no atomic and no wait on another
 * workgroup; max_steps bounds the march and the table size bounds a chain walk: it cannot hang a device.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v or p null, a volume that vk_volume_sample would refuse, a flag other
 * than the two, count < 0, rays null with count > 0, t_out or status null, gradients not 16-byte aligned, max_steps
 * outside 1 .. 65536, t_min or t_max not finite, not 0 <= t_min < t_max. count == 0 returns 0 and launches nothing.
 * (units) L = voxel_length, tr = truncation_length / L, t0 = t_min / L, t1 = t_max / L; with VK_CAST_VOXEL_UNITS
 * t0 = t_min, t1 = t_max and nothing is divided, in the origin or in t. The march runs in voxels.
 * (the ray) ray i is origin x = rays[6i .. 6i+2] and direction d = rays[6i+3 .. 6i+5] (any length), in the frame that
 * pose_dev carries into the volume's. q_a = x_a / L (q = x with VK_CAST_VOXEL_UNITS). With pose_dev == NULL o = q, else
 * o = fwd(q) as vk_volume_sample defines fwd, and the direction goes through the rotation only:
 * d'_a = (m[a] d_0 + m[4+a] d_1) + m[8+a] d_2. len = sqrtf((d_0 d_0 + d_1 d_1) + d_2 d_2), n_a = d_a / len. The ray is
 * VK_RAY_INVALID unless |o_a| < 2^30 for every a (a NaN fails it; beyond the cell clamp below a cell is not the point's),
 * len is finite and every n_a is finite: a zero direction is invalid (0 / 0), and so is one whose squares overflow (its
 * n would be 0 or NaN).
 * (the march) t = t0, armed = false, steps = 0; repeat:
 *  1. !(t < t1): VK_RAY_MISS.
 *  2. steps == max_steps: VK_RAY_STEPS; else ++steps.
 *  3. p_a = o_a + t * n_a (mul, add); a non-finite p_a: VK_RAY_MISS.
 *  4. the cell c_a = (int)floorf(p_a), saturating, clamped to +-2^30; the block B = c >> 3, found by the chain walk,
 *     absent when a coordinate leaves the int16 range.
 *  5. B absent: leave it through its exit face. For each axis with n_a != 0, face_a = (float)(8 B_a + (n_a > 0 ? 8 : 0))
 *     and s_a = (face_a - p_a) / n_a; s = fminf over those axes in x, y, z order, starting from +infinity;
 *     t = t + (fmaxf(s, 0.0f) + 0.5f). (The reference steps a whole block length, tracer.cu:435, and can jump a block's
 *     corner; a query that must not miss geometry does not.)
 *  6. B present: u = voxel (c & 7) of B, observed = (u.distance_weight != 0), sdf = observed ? u.distance : 1.0f
 *     (Voxel::Empty()'s distance, as the reference reads an unobserved voxel). If observed and sdf <= 0.1f and
 *     sdf >= -0.5f (the reference's window, tracer.cu:383) and vk_volume_sample's distance sample exists at p (voxel
 *     units, no pose, the USED rule), sdf = that sample's distance. If observed and sdf > 0: armed = true. If observed
 *     and armed and sdf <= 0: the refinement. Else t = t + (sdf > 0 ? fmaxf(1.0f, tr * sdf) : 1.0f).
 *  A surface is reported only where the ray crosses it from its observed free side: a ray that starts behind a surface
 *  walks out through it and goes on (the reference, whose rays start at the camera, reports the first sdf <= 0).
 * (the refinement, tracer.cu:396-420) t = t + tr * sdf; p = o + t n; if the distance sample exists at p,
 * t = t + tr * its distance. VK_RAY_HIT.
 * (outputs) status[i] is the outcome. t_out[i] = t * L for a hit (t with VK_CAST_VOXEL_UNITS), 0.0f otherwise: the
 * library's "no measurement", like a raycast depth of 0. For a hit, samples[i] and gradients[4i .. 4i+3] are exactly
 * vk_volume_sample's at p_hit = o + t n with voxel units and no pose, in the volume's frame; for any other outcome
 * Voxel::Empty() (distance 1.0f, the rest 0) and four zeros. With VK_CAST_DISTANCE_ONLY the colour fields are 0 and no
 * colour byte of the pool is read.
 * (writes) t_out[i], status[i], samples[i] and gradients[4i ..] for i < count only, each by its own lane; a null
 * optional output is not written. */
VK_API int vk_volume_cast_rays(const vk_volume* v, const float* rays /* device [6*count]: origin, direction */, int32_t count,
    const vk_transform* pose_dev /* optional, device: T_volume_rays */, const vk_cast_params* p,
    float* t_out /* device [count] */, int32_t* status /* device [count] */,
    vk_voxel* samples /* optional, device [count] */, float* gradients /* optional, device [4*count], 16-byte aligned */, void* stream);

/* ---------------------------------------------------------- integrate rays -- */

enum { VK_RAYS_VOXEL_UNITS = 1, VK_RAYS_ONE_OBSERVATION = 2 };

typedef struct vk_integrate_rays_params {
  int32_t flags;               /* VK_RAYS_*; an unknown bit is VK_ERR_ARGUMENT */
  int32_t max_rounds;          /* 0 .. 64 allocation rounds; 0 allocates nothing (update a fixed map) */
  float   r_min, r_max;        /* a ray has a measurement iff r_min <= range <= r_max (false for a NaN); 0 <= r_min < r_max, finite */
  float   max_distance_weight; /* 1 .. 32767 */
  int32_t pad;
} vk_integrate_rays_params;

/* Fuse `count` range measurements along arbitrary rays into the volume: a spinning LiDAR, a fisheye or otherwise distorted
 * depth camera, a sparse or unorganised point cloud, or what vk_volume_cast_rays returned for another volume — (rays, t)
 * feeds in unchanged, t == 0 being "no measurement". No upstream counterpart (the reference fuses only the pixels of one
 * pinhole depth image, which every voxel finds by projecting into it); ref: src/depth_integrator.cu:54-74 for the band test,
 * the min(1, d / truncation) and the running average, src/volume.cu:87-301 for requesting the blocks within one truncation
 * length either side of the measurement, src/volume.cu:304-368 for the handle pass. The definition is this comment;
 * tests/integrate_rays_reference.py states it on the CPU and the device is held to it bit for bit. All arithmetic is fp32,
 * one rounding per operation, no contraction, IEEE division and a correctly rounded square root.
 * PRECONDITIONS: vk_volume_merge's for dst — between SetView calls, no frame announced (the class layers enforce it).
 * ACCESS: rays, ranges and the pose are only read. Everything is enqueued on `stream`, nothing is read back, no workgroup
 * waits on another; the walk is bounded by G below and a chain walk by the table size: it cannot hang a device. `workspace`:
 * vk_volume_integrate_rays_workspace_bytes(main, excess) bytes, 16-byte aligned, need not be initialised.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v, p, counts_dev or workspace null, a volume that vk_volume_merge would
 * refuse, a flag other than the two, max_rounds outside 0 .. 64, a cap outside 1 .. 32767, r_min or r_max not finite or not
 * 0 <= r_min < r_max, count < 0 or count > 1 << 22, rays or ranges null with count > 0, a workspace not 16-byte aligned,
 * truncation_length / voxel_length > 64. count == 0 returns 0, launches nothing and leaves the counters' bytes alone.
 * (units) L = voxel_length, tr = truncation_length / L. The walk runs in voxels.
 * (the ray) ray i is vk_volume_cast_rays' ray word for word: q = x / L (q = x with VK_RAYS_VOXEL_UNITS), o = q or fwd(q)
 * through pose_dev, the direction through the rotation alone, n = d / sqrtf((d_0 d_0 + d_1 d_1) + d_2 d_2), and INVALID by
 * the same rule (|o_a| not < 2^30, a non-finite length or n_a). range_i = ranges[i] is the distance along n in the origin's
 * unit, like r_min and r_max; r = range_i / L (r = range_i with VK_RAYS_VOXEL_UNITS). A valid ray has a measurement iff
 * r_min <= range_i <= r_max; one without is skipped.
 * (the walk) the exact traversal of the cells the ray crosses inside the band: ta = fmaxf(r - tr, 0), tb = r + tr,
 * p_a = o_a + ta * n_a (mul, add), c_a = (int)floorf(p_a), saturating, clamped to +-2^30. Per axis: n_a > 0: step_a = 1,
 * tmax_a = ta + ((float)(c_a + 1) - p_a) / n_a, tdelta_a = 1.0f / n_a; n_a < 0: step_a = -1, tmax_a = ta + ((float)c_a - p_a)
 * / n_a, tdelta_a = 1.0f / fabsf(n_a); n_a == 0: step_a = 0, both +infinity. At most G = 3 * (min((int)ceilf(tb - ta), 1024)
 * + 2) times (the conversion saturates, a NaN gives 0; tb - ta <= 4 tr, so the 1024 is never reached): visit c; a = the axis
 * of the smallest tmax, x before y before z on a tie (tmax_y < tmax_x, then tmax_z < the smaller: a NaN is never smaller);
 * !(tmax_a <= tb): end; c_a += step_a, tmax_a = tmax_a + tdelta_a. A visited cell whose block B = c >> 3 has a coordinate
 * outside the int16 range is passed over: it is requested nowhere, counted nowhere and takes no update.
 * (allocation) vk_volume_merge's rounds with the blocks of the visited cells of the rays that have a measurement in the place
 * of the source blocks: presence by the chain walk, one request per bucket and round, MAIN or EXCESS, the largest key wins, a
 * MAIN request sets visibility TRUE, one vk_volume_handle_allocation_requests per round, the same two ends of the rounds
 * (a round that posts nothing, a round that drops), exhaustion included. max_rounds == 0: no round.
 * (accumulation) for every visited cell whose block is present after the rounds: e_a = (float)c_a + 0.5f,
 * raw = r - (((e_0 - o_0) n_0 + (e_1 - o_1) n_1) + (e_2 - o_2) n_2); if raw > -tr: u = fminf(1.0f, raw / tr),
 * q = (int)rintf(u * 1048576.0f) (ties to even), and the voxel's S += q (a 64-bit integer), N += 1. Integer sums commute:
 * S and N do not depend on the order of the rays or on timing. No float atomic touches a voxel or an accumulator.
 * (the fold) for every voxel with N > 0: m = ((float)S / (float)N) * 0x1p-20f (both conversions round to nearest even),
 * ws = VK_RAYS_ONE_OBSERVATION ? 1.0f : (float)N, and the voxel's running average goes on as vk_volume_merge continues it with
 * a source voxel of distance m and weight ws: wd = (float)distance_weight, distance = wd == 0 ? m : (wd * distance + ws * m)
 * / (wd + ws), distance_weight = (int16)fminf(max_distance_weight, wd + ws). The colour fields and the colour weight keep
 * their bytes; a voxel with N == 0 keeps all its bytes; an allocated block that took no update stays Voxel::Empty().
 * (afterwards) as after vk_volume_merge: VK_CTR_VISIBLE = 0, VK_CTR_BANDED = -1, anything prepared ahead is void.
 * counts_dev int32[8]: rays integrated (valid, with a measurement); valid rays without a measurement; invalid rays; blocks
 * allocated by the call (visited blocks present after the rounds and not before); rounds that posted; blocks that took an
 * update; voxels updated; cell visits lost to a block still absent (counted before the band test; the sum wraps at 2^32). */
VK_API size_t vk_volume_integrate_rays_workspace_bytes(int32_t main, int32_t excess);
VK_API int vk_volume_integrate_rays(const vk_volume* v, const float* rays /* device [6*count]: origin, direction */,
    const float* ranges /* device [count] */, int32_t count, const vk_transform* pose_dev /* optional: T_volume_rays */,
    const vk_integrate_rays_params* p, int32_t* counts_dev /* [8] */, void* workspace, void* stream);

/* Measurement only: the next vk_volume_integrate_rays of this host thread records events[0 .. 5] (vk_event_create) on its
 * stream in front of its first pass, behind the allocation rounds, the mark pass, the zero pass, the add pass and the fold,
 * so that tools/integrate_rays_bench.py can say what each pass costs; no upstream counterpart (ref: the reference times its
 * integrator from outside, src/depth_integrator.cu:89-115). One CALL only, as with vk_integrate_time_next: the events are used
 * up by the next call even when it returns an error before its launches, and a call with count == 0 records none;
 * (NULL, 0) cancels. `count` must be 6. Not a stream operation: nothing is enqueued by this call. */
VK_API int vk_volume_integrate_rays_time_next(void* const* events, int32_t count);

/* -------------------------------------------------------------- carve rays -- */

typedef struct vk_carve_rays_params {
  int32_t flags;               /* VK_RAYS_VOXEL_UNITS | VK_RAYS_ONE_OBSERVATION; any other bit is VK_ERR_ARGUMENT */
  int32_t max_blocks;          /* 1 .. 4096: blocks a ray's carve may cross */
  float   r_min, r_max;        /* a ray has a measurement iff r_min <= range <= r_max (vk_volume_integrate_rays' rule) */
  float   t_from;              /* the carve starts here along the ray, in the origin's unit; finite, >= 0 */
  float   max_distance_weight; /* 1 .. 32767 */
} vk_carve_rays_params;        /* 24 bytes */

/* Carve free space along `count` range rays: every voxel of an existing block whose cell a ray crosses between t_from and the
 * start of the band around its measurement takes one observation of "free", the distance 1 that the reference integrator
 * writes in front of a surface (min(1, d / truncation), ref: src/depth_integrator.cu:54-74). vk_volume_integrate_rays fuses
 * the band and nothing in front of it, so a surface that was fused once and is gone stays until a ray carves it. No upstream
 * counterpart. The definition is this comment; tests/carve_rays_reference.py states it on the CPU and the device is held to
 * it bit for bit. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division and a correctly rounded
 * square root.
 * PRECONDITIONS: vk_volume_integrate_rays' — between SetView calls, no frame announced (the class layers enforce it).
 * ACCESS: rays, ranges, the pose, the hash table are only read; of the volume only voxels are written. THE CALL ALLOCATES
 * NOTHING: the hash table, the free list, the visibility and allocation arrays, the visible list and every VK_CTR_* keep their
 * bytes, and the lists of the last SetView stay valid. Everything is enqueued on `stream`, nothing is read back, no workgroup
 * waits on another; the block walk is bounded by max_blocks, a cell walk by G <= 48 and a chain walk by the table size: it
 * cannot hang a device. `workspace`: vk_volume_carve_rays_workspace_bytes(main, excess) bytes, 16-byte aligned, need not be
 * initialised.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v, p, counts_dev or workspace null, a volume that vk_volume_merge would
 * refuse, a flag other than the two, max_blocks outside 1 .. 4096, a cap outside 1 .. 32767, r_min or r_max not finite or not
 * 0 <= r_min < r_max, t_from not finite or < 0, count < 0 or count > 1 << 22, rays or ranges null with count > 0, a workspace
 * not 16-byte aligned, truncation_length / voxel_length > 64. count == 0 returns 0, launches nothing and leaves counts_dev alone.
 * (the ray) vk_volume_integrate_rays' word for word: units, pose, n, the INVALID rule, r, the measurement test.
 * (the carve interval) tr = truncation_length / L, t0 = t_from / L (t0 = t_from with VK_RAYS_VOXEL_UNITS), te = r - tr. A ray
 * CARVES iff it is valid, has a measurement and t0 < te (false for a NaN; r is finite for a measured ray unless range / L
 * overflows, and te = +infinity then carves up to max_blocks blocks like any long ray).
 * (the block walk) vk_volume_integrate_rays' traversal with a cell edge of 8: p_a = o_a + t0 * n_a, B_a = c_a >> 3 with
 * c_a = (int)floorf(p_a), saturating, clamped to +-2^30. Per axis: n_a > 0: bstep_a = 1, bmax_a = t0 + ((float)(8 (B_a + 1))
 * - p_a) / n_a, bdelta_a = 8.0f / n_a; n_a < 0: bstep_a = -1, bmax_a = t0 + ((float)(8 B_a) - p_a) / n_a, bdelta_a = 8.0f /
 * fabsf(n_a); n_a == 0: bstep_a = 0, both +infinity. t_in = t0. At most max_blocks times: least = the smallest bmax, x before y
 * before z on a tie (bmax_y < bmax_x, then bmax_z < the smaller: a NaN is never smaller); t_out = fminf(least, te); visit
 * block B over [t_in, t_out]; !(least < te): end; B_a += bstep_a, bmax_a = bmax_a + bdelta_a, t_in = least. A ray whose turns
 * run out first is CUT SHORT: what it did not reach is not carved.
 * (visiting a block) a block with a coordinate outside the int16 range, or absent from the table (the chain walk), is passed
 * over. A present block runs vk_volume_integrate_rays' cell walk with ta = t_in and tb = t_out: the same p, c, tmax, tdelta,
 * tie rule and guard G = 3 * (min((int)ceilf(tb - ta), 1024) + 2), the conversion saturating and a NaN giving 0 (tb - ta is at
 * most a block's diagonal, under 14, so G <= 48 for finite ends; a non-finite difference meets the clamp at 1024, never int
 * arithmetic). A visited cell c takes a carve iff c >> 3 == B on all three axes and the walk leaves it before the band begins:
 * least' <= te, least' the smallest tmax right after the visit (the walk's own next test is least' <= tb). The cell that
 * straddles te is the band walk's, which starts inside it.
 * (accumulation) a carve adds 1 to the voxel's 32-bit count N (N <= count <= 2^22). Every carve observes min(1, raw / tr) for
 * raw > tr, exactly 1: there is no sum and nothing to quantise. No float atomic touches a voxel or an accumulator.
 * (the fold) for every voxel with N > 0: ws = VK_RAYS_ONE_OBSERVATION ? 1.0f : (float)N, wd = (float)distance_weight,
 * distance = wd == 0 ? 1.0f : (wd * distance + ws) / (wd + ws), distance_weight = (int16)fminf(max_distance_weight, wd + ws).
 * The colour fields and the colour weight keep their bytes; a voxel with N == 0 keeps all its bytes.
 * counts_dev int32[8]: rays that carved; measured rays with nothing to carve (!(t0 < te)); valid rays without a measurement;
 * invalid rays; rays cut short by max_blocks; blocks that took an update; voxels updated; carves (the sum of all N, wrapping
 * at 2^32). */
VK_API size_t vk_volume_carve_rays_workspace_bytes(int32_t main, int32_t excess);
VK_API int vk_volume_carve_rays(const vk_volume* v, const float* rays /* device [6*count]: origin, direction */,
    const float* ranges /* device [count] */, int32_t count, const vk_transform* pose_dev /* optional: T_volume_rays */,
    const vk_carve_rays_params* p, int32_t* counts_dev /* [8] */, void* workspace, void* stream);

/* -------------------------------------------------------------- color rays -- */

typedef struct vk_color_rays_params {
  int32_t flags;               /* VK_RAYS_VOXEL_UNITS | VK_RAYS_ONE_OBSERVATION; any other bit is VK_ERR_ARGUMENT */
  float   r_min, r_max;        /* a ray has a measurement iff r_min <= range <= r_max (vk_volume_integrate_rays' rule) */
  float   band;                /* half width of the coloured stretch around the measurement, in the origin's unit; > 0, finite */
  float   max_color_weight;    /* 1 .. 32767 */
  int32_t pad;
} vk_color_rays_params;        /* 24 bytes */

/* Fuse a colour per range ray into the volume: every voxel of an existing block whose cell a coloured ray crosses within
 * `band` of its measurement, and whose stored distance says it is near the surface, continues its colour's running average
 * with the mean colour of the rays through it — a LiDAR return coloured by a camera, or the colour vk_volume_cast_rays
 * returned for another volume. vk_volume_integrate_rays and vk_volume_carve_rays leave the colour alone; this call writes
 * nothing else. No upstream counterpart (the reference colours only from the pixels of one pinhole image); ref:
 * src/color_integrator.cu:121 for the test that a voxel is near the surface, src/color_integrator.cu:125-129 for the running
 * average and its cap. The definition is this comment; tests/color_rays_reference.py states it on the CPU and the device is
 * held to it bit for bit. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division and a correctly
 * rounded square root.
 * PRECONDITIONS: vk_volume_integrate_rays' — between SetView calls, no frame announced (the class layers enforce it).
 * ACCESS: rays, ranges, colors, the pose, the hash table are only read; of the volume only the colour and the colour weight
 * of voxels are written. THE CALL ALLOCATES NOTHING: the hash table, the free list, the visibility and allocation arrays, the
 * visible list and every VK_CTR_* keep their bytes, and the lists of the last SetView stay valid; so do distance and
 * distance_weight of every voxel. Everything is enqueued on `stream`, nothing is read back, no workgroup waits on another; the
 * walk is bounded by G <= 390 and a chain walk by the table size: it cannot hang a device. `workspace`:
 * vk_volume_color_rays_workspace_bytes(main, excess) bytes (16 per pool voxel), 16-byte aligned, need not be initialised.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): v, p, counts_dev or workspace null, a volume that vk_volume_merge would
 * refuse, a flag other than the two, a cap outside 1 .. 32767, r_min or r_max not finite or not 0 <= r_min < r_max, band not
 * finite or <= 0 or band / L > 64 (band > 64 with VK_RAYS_VOXEL_UNITS), count < 0 or count > 1 << 21, rays, ranges or colors
 * null with count > 0, a workspace not 16-byte aligned, truncation_length / voxel_length > 64. count == 0 returns 0, launches
 * nothing and leaves counts_dev alone.
 * (the ray) vk_volume_integrate_rays' word for word: units, pose, n, the INVALID rule, r, the measurement test.
 * (has a colour) c_k = colors[3i + k]. A measured ray HAS A COLOUR iff 0 <= c_k <= 1 for all three channels (false for a
 * NaN). A ray is, by the first that applies: invalid; without a measurement; without a colour; COLOURED. Only a coloured
 * ray walks.
 * (the walk) b = band / L (b = band with VK_RAYS_VOXEL_UNITS), ta = fmaxf(r - b, 0), tb = r + b, and from there
 * vk_volume_integrate_rays' cell walk unchanged: the same p, c, tmax, tdelta, tie rule and guard G = 3 * (min((int)ceilf(tb -
 * ta), 1024) + 2), the conversion saturating and a NaN giving 0 (tb - ta <= 2 b <= 128, so G <= 390 for finite ends). A
 * visited cell whose block B = c >> 3 has a coordinate outside the int16 range is passed over: counted nowhere. A visited
 * cell whose block is absent from the table (the chain walk) is a LOST visit: counted, and skipped.
 * (accumulation) every other visit adds q_k = (int)rintf(c_k * 1024.0f) (ties to even) to the voxel's three sums S_k and 1 to
 * its N. With count <= 2^21 and c_k <= 1 every S_k <= 2^31 and N <= 2^21: two 64-bit words per voxel, S_0 | S_1 << 32 and
 * S_2 | N << 32, hold the four with no carry between them, and a visit is two 64-bit integer atomics. Integer sums commute:
 * S_k and N do not depend on the order of the rays or on timing. No float atomic touches a voxel or an accumulator.
 * (the fold) for every voxel with N > 0: it is NEAR THE SURFACE iff fabsf(distance) < 1.0f, the stored distance (false for
 * a NaN; a voxel nothing was fused into holds 1). A near voxel: m_k = ((float)S_k / (float)N) * 0x1p-10f (both conversions
 * exact or round to nearest even), ws = VK_RAYS_ONE_OBSERVATION ? 1.0f : (float)N, wc = (float)color_weight, color_k =
 * wc == 0 ? m_k : (wc * color_k + ws * m_k) / (wc + ws), color_weight = (int16)fminf(max_color_weight, wc + ws):
 * vk_volume_merge's continuation with the reference's cap. A voxel that is not near is counted and keeps all its bytes, as
 * does every voxel with N == 0.
 * counts_dev int32[8]: rays coloured; measured rays without a colour; valid rays without a measurement; invalid rays; blocks
 * that took an update; voxels updated; voxels visited (N > 0) but not near the surface; visits lost to an absent block (the sum
 * wraps at 2^32). */
VK_API size_t vk_volume_color_rays_workspace_bytes(int32_t main, int32_t excess);
VK_API int vk_volume_color_rays(const vk_volume* v, const float* rays /* device [6*count]: origin, direction */,
    const float* ranges /* device [count] */, const float* colors /* device [3*count]: r, g, b in [0, 1] */, int32_t count,
    const vk_transform* pose_dev /* optional: T_volume_rays */, const vk_color_rays_params* p, int32_t* counts_dev /* [8] */,
    void* workspace, void* stream);

/* Measurement only: the next vk_volume_color_rays of this host thread records events[0 .. 4] (vk_event_create) on its stream
 * in front of its first pass, behind the mark pass, the zero pass, the add pass and the fold, so that
 * tools/color_rays_bench.py can say what each pass costs; no upstream counterpart (ref: the reference times its integrators
 * from outside, src/color_integrator.cu:144-148). One CALL only, as with
 * vk_volume_integrate_rays_time_next: the events are used up by the next call even when it returns an error before its
 * launches, and a call with count == 0 records none; (NULL, 0) cancels. `count` must be 5. Not a stream operation. */
VK_API int vk_volume_color_rays_time_next(void* const* events, int32_t count);

/* ----------------------------------------------------------- register rays -- */

typedef struct vk_register_rays_params {
  int32_t flags;             /* VK_RAYS_VOXEL_UNITS; any other bit VK_ERR_ARGUMENT */
  int32_t iterations;        /* 1 .. 64 */
  float   r_min, r_max;      /* a ray has a measurement iff r_min <= range <= r_max (vk_volume_integrate_rays' rule) */
  float   max_abs_distance;  /* band, in truncation lengths: 0 < band <= 1 */
  int32_t pad;
} vk_register_rays_params;   /* 24 bytes */

/* Localise a sweep of range rays in the volume: refine the sensor's pose T_volume_rays — the pose vk_volume_integrate_rays,
 * vk_volume_carve_rays and vk_volume_color_rays take as given — by Gauss-Newton on "the endpoint of a return lies on the
 * mapped surface": every measured ray's endpoint is carried into the volume, the field is sampled there, and the pose moves
 * so that the sample is 0. It REFINES a guess that already brings the endpoints within roughly a truncation length of the
 * surface; it searches nothing. No upstream counterpart (the reference tracks pinhole depth images against a raycast
 * keyframe); ref: src/tracker.cpp:124-163 for the loop and its end, src/color_tracker.cpp:45-95 for the step,
 * src/tracer.cu:238-299 for the trilinear sample. The definition is this comment; tests/register_rays_reference.py states
 * it on the CPU. All arithmetic is fp32, one rounding per operation, no contraction, IEEE division and a correctly rounded
 * square root.
 * ACCESS: the volume, rays and ranges are only read: the call may run while a frame is announced, like vk_volume_sample.
 * HOST CHECKS (VK_ERR_ARGUMENT, nothing enqueued): v, p, pose_dev, an output (update_dev alone may be null) or the workspace
 * null, a volume that vk_volume_sample would refuse, a flag other than VK_RAYS_VOXEL_UNITS, iterations outside 1 .. 64, the
 * band not in (0, 1] (a NaN included), r_min or r_max not finite or not 0 <= r_min < r_max, count < 0 or count > 1 << 22,
 * rays or ranges null with count > 0, a workspace not 16-byte aligned. count == 0 returns 0, launches nothing and leaves
 * every output's bytes alone.
 * (the ray) vk_volume_integrate_rays' word for word: units, pose_dev = T_volume_rays, n, the INVALID rule, r, the
 * measurement test. Here pose_dev is required: it is the unknown. m is used as given; the solve rewrites m and inv together.
 * (endpoint) of a valid ray with a measurement: e_a = o_a + r * n_a (mul, add), in voxels, in the volume's frame. A measured
 * ray with a non-finite e_a has no sample.
 * (sample) vk_volume_register's at p = e: g_a = e_a - 0.5f, b_a = floorf(g_a), f_a = g_a - b_a, the eight lattice points
 * b + k found by the chain walk, absent when a block coordinate leaves the int16 range; the sample exists iff all eight are
 * present with distance_weight != 0 (no "used points" rule); D and gx, gy, gz by the very lerp sequence written there.
 * (residual) exists iff the ray is valid and measured, the sample exists and fabsf(D) < band. Then r_i = D — the endpoint
 * of a return lies on the surface, so the target is 0 — weight 1,
 *   J0 = e1*gz - e2*gy, J1 = e2*gx - e0*gz, J2 = e0*gy - e1*gx,  J3 = gx*iv, J4 = gy*iv, J5 = gz*iv,
 * iv = 1.0f / voxel_length computed once: vk_volume_register's form; the unknown is a twist applied on the left of
 * T_volume_rays, in the volume's frame. THE BAND IS THE ONLY OUTLIER RULE: a return further than `band` truncation lengths
 * from the mapped surface (a moved object, a spurious return) takes no part; there are no per-ray weights and no robust loss.
 * (system) vk_volume_register's layout: system[0..21) the packed lower triangle of sum J J^T, system[36..42) sum J r,
 * system[42] sum r^2, the rest 0. A workgroup owns a fixed run of consecutive rays and writes its row of partial sums
 * whatever it found; one workgroup then adds the rows in a fixed order. The order depends on `count` alone: the same inputs
 * give the same bytes every call. counts_dev = {valid rays with a measurement, of those with a sample, residuals, invalid
 * rays}.
 * (step, state, end of the loop) vk_volume_register's, word for word: state_dev = {steps run, code} zeroed by the caller;
 * code 1 when |update| < 1e-6; VK_REGISTER_NO_OVERLAP when a step has no residual, which counts as a step, leaves the
 * pose's bytes alone and writes a zero update; an update of six zeros leaves the pose's bytes alone. A sweep that sees a
 * single plane gives a rank-deficient system: the library's LDL^T answers that with the zero update, so the loop ends with
 * code 1 at the pose it had — the caller must judge observability from the scene.
 * vk_volume_register_rays enqueues `iterations` steps on `stream`, launch per stage (the residual pass, the sum, a one-wave
 * solve), nothing read back. Nothing waits on another workgroup, there is no float atomic and a chain walk is bounded by
 * the table size: it cannot hang a device. A stage that finds state_dev[1] != 0 returns at once, so system_dev and
 * counts_dev hold the last evaluated step's values, those of the pose BEFORE that step's update.
 * vk_volume_register_rays_system: one evaluation at the pose. vk_volume_register_rays_terms: valid[i], residuals[i] and
 * jacobians[6i ..] of ray i, zeros where no residual exists; nothing past `count` is written.
 * workspace: device, vk_volume_register_rays_workspace_bytes(count) bytes (0 for a count the call would refuse), 16-byte
 * aligned, need not be initialised. */
/* ref: src/tracker.cpp:124-163 (the loop whose sums this sizes; no upstream counterpart) */
VK_API size_t vk_volume_register_rays_workspace_bytes(int32_t count);
/* ref: src/tracer.cu:238-299 (the trilinear sample of every term; no upstream counterpart). rays: device [6*count], origin and
 * direction; ranges: device [count]; pose_dev: T_volume_rays; residuals [count], jacobians [6*count], valid [count]. */
VK_API int vk_volume_register_rays_terms(const vk_volume* v, const float* rays, const float* ranges, int32_t count,
    const vk_transform* pose_dev, const vk_register_rays_params* p, float* residuals, float* jacobians, uint8_t* valid,
    void* workspace, void* stream);
/* ref: src/tracker.cpp:124-163 (one evaluation of the loop's system; no upstream counterpart). system_dev [48], counts_dev [4]. */
VK_API int vk_volume_register_rays_system(const vk_volume* v, const float* rays, const float* ranges, int32_t count,
    const vk_transform* pose_dev, const vk_register_rays_params* p, float* system_dev, int32_t* counts_dev, void* workspace,
    void* stream);
/* ref: src/tracker.cpp:124-163 for the loop and its end, src/color_tracker.cpp:45-95 for the step (no upstream counterpart).
 * pose_dev in: the start, out: the result; system_dev [48], state_dev [2], counts_dev [4], update_dev optional [6]. */
VK_API int vk_volume_register_rays(const vk_volume* v, const float* rays, const float* ranges, int32_t count, vk_transform* pose_dev,
    const vk_register_rays_params* p, float* system_dev, int32_t* state_dev, int32_t* counts_dev, float* update_dev, void* workspace,
    void* stream);

/* ------------------------------------------------------------- score poses -- */

typedef struct vk_score_poses_params {
  int32_t flags;             /* VK_RAYS_VOXEL_UNITS; any other bit VK_ERR_ARGUMENT */
  int32_t min_residuals;     /* >= 1: vk_volume_score_poses_best names no pose with fewer */
  float   r_min, r_max;      /* a ray has a measurement iff r_min <= range <= r_max (vk_volume_integrate_rays' rule) */
  float   max_abs_distance;  /* band, in truncation lengths: 0 < band <= 1 */
  int32_t pad;
} vk_score_poses_params;     /* 24 bytes */

typedef struct vk_pose_score {
  int32_t measured, sampled, residuals, invalid;  /* vk_volume_register_rays' four counts at this pose */
  int64_t sum_abs;           /* sum over residuals of (int64) rintf(fabsf(D) * 1048576.0f) */
  int64_t sum_squares;       /* sum over residuals of (int64) rintf((D * D) * 1048576.0f) */
} vk_pose_score;             /* 32 bytes */

/* Score many candidate poses T_volume_rays for one sweep of range rays, and name the one that explains the sweep best: the
 * start vk_volume_register_rays needs and cannot find — a sensor switched on somewhere in a known map, a tracker that lost
 * its pose, a loop-closure candidate to verify. It evaluates vk_volume_register_rays' residual test at every (pose, ray)
 * pair; producing the candidates (a grid, a sampler) is the caller's. No upstream counterpart (the reference tracks pinhole
 * depth images against a raycast keyframe); ref: src/tracker.cpp:124-163 for the loop whose start this finds,
 * src/color_tracker.cpp:45-95 for the step, src/tracer.cu:238-299 for the trilinear sample. The definition is this comment;
 * tests/score_poses_reference.py states it on the CPU. The float arithmetic is vk_volume_register_rays'.
 * ACCESS: the volume, rays, ranges and poses are only read: the calls may run while a frame is announced, like
 * vk_volume_sample and vk_volume_register_rays.
 * HOST CHECKS (VK_ERR_ARGUMENT, nothing enqueued): vk_volume_register_rays' (v, p, poses_dev, scores_dev or the workspace
 * null, a volume that vk_volume_sample would refuse, a flag other than VK_RAYS_VOXEL_UNITS, the band not in (0, 1], r_min or
 * r_max not finite or not 0 <= r_min < r_max, count < 0 or count > 1 << 22, rays or ranges null with count > 0, a workspace
 * not 16-byte aligned), and pose_count outside 1 .. 65 536, (int64) count * pose_count > 1 << 28 (one call stays bounded on
 * a shared machine), min_residuals < 1. count == 0 returns 0, launches nothing and leaves every output's bytes alone.
 * (pair) for pose k and ray i the terms are vk_volume_register_rays' word for word with poses_dev[k] as T_volume_rays: the
 * ray, its INVALID rule and its measurement test, the endpoint, the sample, and the residual test fabsf(D) < band. D is the
 * very float32 vk_volume_register_rays_terms writes to residuals[i] at that pose. No Jacobian, no gradient.
 * (score) scores_dev[k] = {valid rays with a measurement, of those with a sample, residuals, invalid rays} — what
 * vk_volume_register_rays_system writes to counts_dev at that pose — and, over the residuals, sum_abs and sum_squares as
 * written at vk_pose_score: float32 products (the one with 2^20 is exact), rintf, then INTEGER sums. They commute, so a score
 * does not depend on how pairs are dealt to lanes, waves and workgroups, or on timing: the same inputs give the same bytes,
 * and permuted rays give the same score. A term is <= 2^20, a wave's sum <= 2^26, a pose's <= 2^42. The mean |D| of pose k
 * is sum_abs / 2^20 / residuals and its rms sqrtf(sum_squares / 2^20 / residuals), in truncation lengths, each term within
 * half a unit (2^-21).
 * (shape) a workgroup owns 256 consecutive rays x 8 consecutive poses, one lane per ray looping over the poses, and writes
 * its partial scores whatever it found; a second launch adds them per pose. Nothing waits on another workgroup, there is no
 * atomic and a chain walk is bounded by the table size: it cannot hang a device. Every vk_pose_score up to pose_count is
 * written, nothing beyond; scores_dev needs no initial contents.
 * workspace: device, vk_volume_score_poses_workspace_bytes(count, pose_count) bytes (0 for a shape the call would refuse),
 * 16-byte aligned, need not be initialised.
 * vk_volume_score_poses_best: one small launch. The best pose is the one with the most residuals, then the smallest
 * sum_abs, then the smallest index: a total order. If it has residuals >= p->min_residuals, best_dev[0] = its index k and
 * poses_dev[k]'s 128 bytes are copied to pose_out_dev; otherwise best_dev[0] = -1 and pose_out_dev's bytes are left alone.
 * vk_volume_register_rays can be enqueued from pose_out_dev right behind it: score, choose, refine is one enqueue with no
 * host round trip (after a -1 it refines whatever pose_out_dev held: read best_dev before trusting the result). HOST CHECKS:
 * a null pointer, pose_count outside 1 .. 65 536, a flag other than VK_RAYS_VOXEL_UNITS, min_residuals < 1; the rest of p
 * is not used. */
/* ref: src/tracker.cpp:124-163 (the loop whose candidate starts this sizes; no upstream counterpart) */
VK_API size_t vk_volume_score_poses_workspace_bytes(int32_t count, int32_t pose_count);
/* ref: src/tracer.cu:238-299 (the trilinear sample of every pair; no upstream counterpart). rays: device [6*count], origin and
 * direction; ranges: device [count]; poses_dev: device [pose_count] T_volume_rays; scores_dev: device [pose_count]. */
VK_API int vk_volume_score_poses(const vk_volume* v, const float* rays, const float* ranges, int32_t count,
    const vk_transform* poses_dev, int32_t pose_count, const vk_score_poses_params* p, vk_pose_score* scores_dev, void* workspace,
    void* stream);
/* ref: src/tracker.cpp:124-163 (the loop this chooses the start of; no upstream counterpart). best_dev: device int32[1];
 * pose_out_dev: device vk_transform. */
VK_API int vk_volume_score_poses_best(const vk_pose_score* scores_dev, const vk_transform* poses_dev, int32_t pose_count,
    const vk_score_poses_params* p, int32_t* best_dev, vk_transform* pose_out_dev, void* stream);

/* ---------------------------------------------------------- clearance field -- */

enum { VK_CELL_UNKNOWN = 1, VK_CELL_FREE = 2, VK_CELL_OCCUPIED = 4 };
enum { VK_FIELD_SIGNED = 1 };
#define VK_FIELD_BEYOND INT32_MAX   /* d2 of a cell with no site within max_cells */

typedef struct vk_cell_grid {
  int32_t origin[3];         /* lattice coordinates of the grid's first voxel, each a multiple of stride, |origin| <= 2^20 */
  int32_t dims[3];           /* cells per axis, 1 .. 1024 each, nx * ny * nz <= 2^27 */
  int32_t stride;            /* voxels per cell and axis: 1, 2, 4 or 8 */
  int32_t pad;
} vk_cell_grid;              /* 32 bytes */

typedef struct vk_distance_field_params {
  int32_t flags;             /* 0 or VK_FIELD_SIGNED; an unknown bit is VK_ERR_ARGUMENT */
  int32_t site_mask;         /* 1 .. 7: VK_CELL_* or'ed, the classes a distance is measured to */
  int32_t max_cells;         /* 1 .. 256: the cap of the search, in cells */
  float   occupied_below;    /* finite, in [-1, 1], truncation lengths; 0: the zero crossing */
} vk_distance_field_params;  /* 16 bytes */

/* How far is a place from the nearest surface: the hashed volume classified into a dense grid of cells, and the exact
 * Euclidean distance transform of that grid. The stored distance saturates at one truncation length; a planner needs metres
 * of clearance, densely, over a box. No upstream counterpart (the reference never leaves its truncation band; ref:
 * src/volume.cu:168-191 for the chain walk). The definition is this comment; tests/distance_field_reference.py states it on
 * the CPU and the device is held to it bit for bit: the classes and the squared distances are integers, and the float field is
 * fp32 with one rounding per operation, a correctly rounded square root and no contraction.
 * ACCESS: the volume is only read: the calls are allowed while a frame is announced, like vk_volume_sample. No atomic and
 * no wait on another workgroup; a chain walk is bounded by the table, everything else by dims and max_cells: they cannot
 * hang a device. Nothing is read back. Every call initialises what it reads of the workspace, and writes only the arrays
 * it was given, elements [0, nx*ny*nz) of each.
 * (grid) cell (i, j, k), 0 <= i < dims[0], 0 <= j < dims[1], 0 <= k < dims[2], covers the stride^3 voxels
 * n_a = origin_a + stride * idx_a + e_a, 0 <= e_a < stride, in lattice coordinates as vk_volume_sample numbers them: n is
 * voxel (n mod 8) — index z*64 + y*8 + x — of block floor(n / 8), found by the chain walk; the block is absent when a
 * coordinate leaves the int16 range. As every origin_a is a multiple of stride, a cell lies in one block. Arrays are indexed
 * (k * ny + j) * nx + i, x fastest.
 * (class of a cell, one uint8_t) a voxel is OBSERVED iff its block is present and distance_weight != 0; it is OCCUPIED iff it
 * is observed and distance <= occupied_below (an fp32 compare of the stored value; a NaN is not occupied). A cell is
 * VK_CELL_OCCUPIED iff one of its voxels is occupied, else VK_CELL_FREE iff one of its voxels is observed, else
 * VK_CELL_UNKNOWN. This map allocates blocks only inside the truncation band: open space in front of the band has no blocks
 * and reads UNKNOWN, not FREE (vk_volume_carve_rays observes it). The clearance field, whose sites are the occupied cells,
 * does not depend on that.
 * (transform) a cell is a SITE iff class & site_mask != 0. d2(p) is the minimum of |p - q|^2 over the sites q of the grid,
 * in cells, an integer; it is VK_FIELD_BEYOND where the grid has no site or where that minimum exceeds max_cells^2. Cells
 * outside the grid do not exist. (Three separable passes along x, y and z that search only offsets within max_cells and drop
 * what exceeds max_cells^2 give exactly this: a nearest site within the cap is within the cap on every axis.)
 * (float field) distance = (sqrtf((float)d2) * (float)stride) * voxel_length, +INFINITY where d2 is VK_FIELD_BEYOND;
 * (float)d2 is exact, d2 <= 65536. With VK_FIELD_SIGNED a site cell takes -((sqrtf((float)e2) * (float)stride) * voxel_length)
 * instead, e2 being the same transform with the complement mask 7 ^ site_mask, and -INFINITY where e2 is VK_FIELD_BEYOND
 * (e2 >= 1 at a site). d2 is the unsigned transform's in either case.
 * HOST CHECKS (VK_ERR_ARGUMENT, no device touched): a null pointer that is not optional, a volume that vk_volume_sample would
 * refuse, a stride other than 1, 2, 4 or 8, an origin that is not a multiple of the stride or beyond +-2^20, a dim outside
 * 1 .. 1024 or more than 2^27 cells, site_mask outside 1 .. 7, max_cells outside 1 .. 256, an unknown flag, occupied_below
 * not finite or outside [-1, 1], d2 or distance not 4-byte aligned, a workspace not 16-byte aligned.
 * vk_volume_classify_cells: one fill of the grid with UNKNOWN, then one wave per table entry whose block meets the grid
 * reduces the block's stride^3 groups and stores that block's cells; a cell has one owner block, so no atomic and no order.
 * vk_grid_distance_transform: classes -> d2, three launches. workspace: vk_grid_distance_transform_workspace_bytes(dims)
 * bytes (0 for dims outside the limits), need not be initialised.
 * vk_volume_distance_field: the two calls and the conversion in one enqueue. classes and d2 are optional outputs and are
 * exactly what the two separate calls write; with d2 == NULL the last pass writes the floats and no int32 grid reaches
 * memory but the passes' own intermediate. workspace: vk_volume_distance_field_workspace_bytes(grid, p) bytes (0 for a grid
 * or parameters the call would refuse), need not be initialised. */
VK_API int vk_volume_classify_cells(const vk_volume* v, const vk_cell_grid* grid, float occupied_below,
    uint8_t* classes /* device [nx*ny*nz] */, void* stream);
/* ref: none (no upstream counterpart: the reference has no dense grid). The bytes of the workspace for a grid of these dims. */
VK_API size_t vk_grid_distance_transform_workspace_bytes(const int32_t dims[3]);
/* ref: none (no upstream counterpart). classes: device uint8 [nx*ny*nz]; d2: device int32 [nx*ny*nz], 4-byte aligned. */
VK_API int vk_grid_distance_transform(const uint8_t* classes, const int32_t dims[3], int32_t site_mask, int32_t max_cells,
    int32_t* d2, void* workspace, void* stream);
/* ref: none (no upstream counterpart). The same bytes as vk_grid_distance_transform_workspace_bytes(grid->dims). */
VK_API size_t vk_volume_distance_field_workspace_bytes(const vk_cell_grid* grid, const vk_distance_field_params* p);
/* ref: src/volume.cu:168-191 (the chain walk that finds a cell's block; no upstream counterpart). classes (optional) and
 * distance: device [nx*ny*nz]; d2 (optional): device int32 [nx*ny*nz]; d2 and distance 4-byte aligned. */
VK_API int vk_volume_distance_field(const vk_volume* v, const vk_cell_grid* grid, const vk_distance_field_params* p,
    uint8_t* classes, int32_t* d2, float* distance, void* workspace, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* VK_H_ */
