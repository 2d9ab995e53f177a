// vmas_lidar_vjp.h - what the library's host code (vmas_hip.hip) and the translation unit of the LIDAR's backward kernel
// (vmas_lidar_vjp.hip) share: the registered sensor set as the planner reads it, and the plan - the refusal or the table
// the kernel reads, the tile's LDS layout and the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace vmas {
namespace lidar_vjp {

// (the fields of DevLidar / DevTarget, vmas_env_device.h, that the cast reads)
struct Sensor { int32_t entity, n_rays, n_targets, target_off, angle_off; float max_range, half_range; };
struct Target { int32_t entity, shape; float length, width, radius; };

struct Plan {
  bool ok = false;
  char why[320] = "";  // the refusal (ok == false)
  int n_lidars = 0, max_rays = 0, n_slots = 0;  // slots: the entities that cast or are seen
  int n_units = 0, unit_rays = 0;               // work units (sensor, ray chunk) and the rays of a chunk (a multiple of 4)
  int n_runs = 0, nw = 1;                       // runs of sensors between two block barriers; waves per 64-environment tile
  int n_rows = 0;                               // LDS rows of the tile (64 floats each)
  size_t lds_bytes = 0;
  int o_slot = 0, o_sens = 0, o_unit = 0, o_run = 0, o_cur = 0, o_ref = 0;  // word offsets into the table
  std::vector<uint32_t> table;
  uint32_t* d_table = nullptr;
};

// Host only: fills `out` (ok, or why not) for the sensor set as vmas_world_set_lidars was given it.  `angles`: every
// registered ray's angle, sensor after sensor (Sensor::angle_off indexes it).
void make_plan(const Sensor* sensors, int n, const Target* targets, const float* angles, int n_entities, Plan* out);
int upload(Plan* p);    // the table to the current device; 0 / -1 + vmas_last_error
void release(Plan* p);  // hipFree of the table
// One launch on `s`: allocates nothing, never waits.  0 / -1 + vmas_last_error.  `angles_cs`: cos, sin of every registered
// ray at rotation 0 as the forward's lidar_table_kernel made them.
int launch(const Plan& p, int device, int batch, const float2* angles_cs, const float* state, long ld, const float* g_out,
           float* g_state, hipStream_t s);

}  // namespace lidar_vjp
}  // namespace vmas
