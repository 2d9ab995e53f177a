// vmas_vjp.h - what the library's host code (vmas_hip.hip) and the translation unit of the backward kernel
// (vmas_vjp.hip) share: the world's constants the vector-Jacobian product of World.step needs, and its plan - the
// refusal or the table the kernel reads, the tile's LDS layout and the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vmas_hip.h"

namespace vmas {
namespace vjp {

struct WorldConst {
  int32_t substeps;
  float sub_dt, gx, gy;
  int32_t has_gravity;
  float xs, ys;  // NaN = unbounded
  float k, c_coll;
};

struct Plan {
  bool ok = false;
  char why[320] = "";  // the refusal (ok == false)
  WorldConst C{};
  int nE = 0, nA = 0, nP = 0;
  int nw = 1;                     // waves per 64-environment tile
  bool shapes = false;            // a kept pair is line-sphere or box-sphere: the kernel with their code is launched
  int chunk = 0, n_chunks = 0;    // pairs of the largest run between two block barriers (sizes nw), and how many runs there are
  int row_pairs = 0, n_rows = 0;  // first pair row / rows of the tile (64 floats each)
  size_t lds_bytes = 0;
  int o_ent = 0, o_pair = 0, o_ref = 0, o_cur = 0, o_chk = 0;  // word offsets into the table
  std::vector<uint32_t> table;
  uint32_t* d_table = nullptr;
};

// Host only: fills `out` (ok, or why not) for the world as vmas_world_create was given it.
void make_plan(const WorldConst& C, const VmasEntityDesc* ents, int nE, int nA, const VmasPairDesc* pairs, int nP, int n_joints,
               Plan* out);
int upload(Plan* p);    // the table to the current device; 0 / -1 + vmas_last_error
void release(Plan* p);  // hipFree of the table
// One launch on `s`: allocates nothing, never waits.  0 / -1 + vmas_last_error.
int launch(const Plan& p, int device, int batch, const float* state_in, const float* ft_in, long ld, const float* g_state_out,
           const float* g_ft_out, float* g_state_in, float* g_ft_in, hipStream_t s);

}  // namespace vjp
}  // namespace vmas
