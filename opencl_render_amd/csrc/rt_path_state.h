// rt_path_state.h -- where a path's ring entries live inside RtWavefront::ring ("Round 9"), with no HIP in it: the kernels
// of rt_wavefront.hip and tests/path_state_host.cpp (which compiles it for the host on its own) use these functions, so that what the
// test checks is what the device addresses.  Indices are in quads (float4, 16 bytes); the allocation holds RT_PATH_RING_QUADS * capacity.
//
// GENERAL LAYOUT (RtDevScene::pathClass == RT_PATH_CLASS_GENERAL): [capacity][RT_RING = 12 slots][3 quads], 576 bytes per path.
//
// CLASS LAYOUT (RT_PATH_CLASS_OPAQUE_DIFFUSE).  A class path only ever uses two things of its ring: the camera ray's direction (slot 0,
// quad 1: wf_primary_kernel stores it, round 0 reads it back) and ONE bounce entry (slot 1, three quads: round 0 spawns it at tail == 1,
// later rounds read it at head == 1).  The same allocation is then addressed path-major:
//   [0, capacity)               the camera directions, one quad per path -- a wave's 64 paths are 8 whole 128-byte lines;
//   [capacity, 5 * capacity)    one 64-byte-pitch bounce record per path, quads 0..2 used, the fourth spare.  capacity is a multiple of
//                               65 536 and the allocation is line-aligned, so a record never straddles a 128-byte line.
// Slots 2.. do not exist in the class; the kernels raise RT_WF_ERR_SPLIT for a path that asks for one and never index it.
#ifndef RT_PATH_STATE_H
#define RT_PATH_STATE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_PATH_HD __host__ __device__ __forceinline__
#else
#define RT_PATH_HD inline
#endif

#define RT_PATH_RING_SLOTS 12 // == RT_RING (rt_device.h; rt_wavefront.hip asserts it)
#define RT_PATH_RING_QUADS (RT_PATH_RING_SLOTS * 3) // quads allocated per path, whichever layout addresses them
#define RT_PATH_CLASS_BOUNCE_SLOT 1u // the one ring slot besides the camera ray's that a class path has

// general layout: quad `quad` (0..2) of ring slot `slot` (0..11) of path `a`
RT_PATH_HD size_t rt_path_ring_quad(uint32_t a, uint32_t slot, uint32_t quad) { return (size_t)a * RT_PATH_RING_QUADS + slot * 3u + quad; }

// class layout: (slot 0, quad 1) = the camera direction; (slot 1, quad 0..2) = the bounce record.  Nothing else exists.
RT_PATH_HD size_t rt_path_class_quad(uint32_t capacity, uint32_t a, uint32_t slot, uint32_t quad)
{
    return slot == 0u ? (size_t)a : (size_t)capacity + 4u * (size_t)a + quad;
}

#endif
