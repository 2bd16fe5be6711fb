// What every kernel file here assumes about the target, in one place.

#pragma once

#include <cstddef>

#define DEV_INLINE __device__ __forceinline__

constexpr size_t LDS_LIMIT = 160 * 1024;   // gfx950: 160 KiB per workgroup
