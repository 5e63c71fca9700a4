// bad_arguments.h — what the *_bad_arguments.cpp programs share: a vk_volume that passes the host checks, addresses that are
// no memory, EXPECT, and the end of main. No GPU is needed or touched: every call the programs make has to return before
// anything is enqueued.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "vk.h"

static int g_failed = 0;
#define EXPECT(code, call) do { const int got__ = (call); if (got__ != (code)) { ++g_failed; \
    std::printf("line %d: expected %d, got %d: %s\n", __LINE__, (code), got__, #call); } } while (0)

static const float kInf = std::numeric_limits<float>::infinity(), kNan = std::nanf("");
static const int32_t kMost = std::numeric_limits<int32_t>::max(), kLeast = std::numeric_limits<int32_t>::min();

// a volume of 8 + 8 blocks, 8 mm voxels and five of them to the truncation length, whose buffers begin at `base`
static vk_volume Volume(uintptr_t base = uintptr_t(1) << 20)
{
  vk_volume v = {};
  void** fields[8] = {reinterpret_cast<void**>(&v.voxels), reinterpret_cast<void**>(&v.hash_entries), reinterpret_cast<void**>(&v.free_voxel_blocks),
      reinterpret_cast<void**>(&v.allocation_types), reinterpret_cast<void**>(&v.allocation_blocks), reinterpret_cast<void**>(&v.block_visibility),
      reinterpret_cast<void**>(&v.visible_blocks), reinterpret_cast<void**>(&v.counters)};
  for (int k = 0; k < 8; ++k) *fields[k] = reinterpret_cast<void*>(base + 4096 * uintptr_t(k));
  v.main_block_count = 8;
  v.excess_block_count = 8;
  v.voxel_length = 0.008f;
  v.truncation_length = 0.04f;
  return v;
}

// addresses that are no memory, one per kind of argument
static const float* const kRays = reinterpret_cast<const float*>(uintptr_t(4096));
static float* const kFloats = reinterpret_cast<float*>(uintptr_t(8192));
static int32_t* const kInts = reinterpret_cast<int32_t*>(uintptr_t(12288));
static void* const kWorkspace = reinterpret_cast<void*>(uintptr_t(16384));
static uint8_t* const kBytes = reinterpret_cast<uint8_t*>(uintptr_t(20480));
static vk_transform* const kPose = reinterpret_cast<vk_transform*>(uintptr_t(24576));

// the end of main: silent and 0 when every call answered as expected
static int Finish(const char* program)
{
  if (g_failed) std::printf("%s: %d failed\n", program, g_failed);
  return g_failed ? 1 : 0;
}
