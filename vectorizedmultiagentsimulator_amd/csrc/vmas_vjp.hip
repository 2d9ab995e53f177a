// vmas_vjp.hip - the backward kernel of World.step for sphere-only worlds: one launch computes the vector-Jacobian
// product of one vmas_world_step (include/vmas_hip.h, vmas_world_step_vjp; DESIGN.md "Backward of World.step").
//
// Lane = environment, a block owns a tile of 64 environments, as the forward does.  The launch
//   1. re-runs the step's substeps from the saved pre-step state with the forward's own device functions (contact_force,
//      clamp_with_norm, clamp_t, rcp_of: vmas_device.h), so every clamp and contact decision has the forward's bits, and
//      checkpoints per movable entity and substep what the reverse sweep needs: the substep's input position and the
//      velocity in front of its clamps (4 rows of 64 floats = 1 KB);
//   2. sweeps the substeps backwards: the integrator's adjoint per entity (entities round-robin over the waves), then the
//      pair adjoint - the exp/log of the softplus, the dominant cost - with pairs round-robin over the waves.
// A pair's result goes to the pair's own two LDS rows; the owner of an entity then adds the rows of its pairs in the
// reference's pair order.  No atomics: two runs on the same inputs are bitwise equal.  When the rows of all pairs do not
// fit beside the checkpoints, the pairs are evaluated in runs ("chunks") of as many as fit, with the owners' sums
// carried in LDS between runs - the order of the additions is the same.  Tiles never talk to each other: the kernel has
// block barriers only and cannot wait on anything.
//
// Rotation needs no checkpoint: rot and ang_vel are linear in the (once clamped) torque, their adjoint over all
// substeps is a closed form evaluated by the entity's owner on its way out.
//
// Tile rows (64 floats each), per entity e at row arow(e):
//   movable:    0,1  forward: force sum carried between chunks   backward: position cotangent
//               2,3  forward: velocity                           backward: velocity cotangent
//               4,5                                              backward: this substep's force cotangent (read by the pairs)
//               6,7  forward: action force (clamped) + gravity   backward: force cotangent summed over the substeps
//               8 + 4 s ...: checkpoint of substep s: pos.x pos.y, pre-clamp vel.x vel.y
//   immovable:  0,1  position cotangent;  2,3  position
// then 2 rows per pair of a chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "vmas_device.h"
#include "vmas_vjp.h"

namespace vmas {
int host_fail(const char* msg);  // vmas_hip.hip: sets vmas_last_error(), returns -1

namespace vjp {
namespace {

constexpr int ROWF = 64;                 // floats per LDS row = environments per tile
constexpr int EW = 20, PW = 8;           // table words per entity / per pair
constexpr int MAX_WAVES = 8;
constexpr size_t kLdsMax = 160 * 1024;   // LDS of one gfx950 CU

struct Args {
  WorldConst C;
  int32_t nE, nP, chunk, n_chunks, row_pairs;
  int32_t o_ent, o_pair, o_ref, o_cur;
  const uint32_t* tab;
};

VD int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct Ent {
  uint32_t flags; int32_t agent_index, arow, prow;  // wave-uniform
  float mass, inertia, one_minus_drag, max_speed, v_range, gx, gy, max_f, f_range, max_t, t_range;
};
VD Ent load_ent(const uint32_t* p) {
  Ent D;
  D.flags = (uint32_t)sgpr((int)p[0]); D.agent_index = sgpr((int)p[1]); D.arow = sgpr((int)p[2]); D.prow = sgpr((int)p[3]);
  D.mass = __uint_as_float(p[5]); D.inertia = __uint_as_float(p[6]); D.one_minus_drag = __uint_as_float(p[7]);
  D.max_speed = __uint_as_float(p[8]); D.v_range = __uint_as_float(p[9]);
  D.gx = __uint_as_float(p[10]); D.gy = __uint_as_float(p[11]);
  D.max_f = __uint_as_float(p[12]); D.f_range = __uint_as_float(p[13]); D.max_t = __uint_as_float(p[14]); D.t_range = __uint_as_float(p[15]);
  return D;
}

// torch.clamp's backward: the cotangent passes on the closed interval
VD float pass_clamp(float x, float r, float g) { return (x >= 0.f - r && x <= r) ? g : 0.f; }

// VJP of clamp_with_norm(t, max_norm) (vmas_device.h): the identity where n <= max, else max * (I / n - t t^T / n^3)
VD v2 clamp_with_norm_vjp(v2 t, float max_norm, v2 g) {
  const float n = vnorm(t);
  if (!__any(n > max_norm)) return g;
  const rcp_t rn = rcp_of(n);
  const float s = vdot(t, g) / rn / rn / rn;
  const v2 r = V((g.x / rn - t.x * s) * max_norm, (g.y / rn - t.y * s) * max_norm);
  return n > max_norm ? r : g;
}

// VJP of contact_force(pa, pb, ...) (vmas_device.h) with respect to d = pa - pb, for the cotangent fb of the force on a:
// f = c g(dist) d with g = pen / dist, pen = k softplus((dist_min - dist) / k), so d pen / d dist = -sigmoid(x) and
// dbar = c (g fb + (g' / dist) (d . fb) d), g' = (pen' - g) / dist; zero wherever the forward zeroes the force.
VD v2 contact_force_vjp(v2 pa, v2 pb, float dist_min, float c, float k, v2 fb) {
  const v2 d = pa - pb;
  const float dist = vnorm(d);
  if (!__any(!(dist > dist_min))) return V(0.f, 0.f);
  const float x = (dist_min - dist) / rcp_of(k);
  const float pen = softplus0(x) * k;
  const rcp_t den = rcp_of(dist > 0.f ? dist : 1e-8f);
  const float sig = 1.f / rcp_of(1.f + expf(0.f - x));  // (x >= 0 wherever the result is kept)
  const float g = pen / den;
  const float gp = ((0.f - sig) - g) / den;
  const float s = (gp / den) * vdot(d, fb);
  const v2 r = V(c * (g * fb.x + s * d.x), c * (g * fb.y + s * d.y));
  const bool zero = (dist < 1e-6f) || (dist > dist_min);
  return zero ? V(0.f, 0.f) : r;
}

// _apply_action_force's clamps (core.py:2018-2028), as step_kernel applies them
VD v2 clamp_force(const Ent& D, v2 f) {
  if (D.flags & VMAS_F_MAX_F) f = clamp_with_norm(f, D.max_f);
  if (D.flags & VMAS_F_F_RANGE) f = V(clamp_t(f.x, D.f_range), clamp_t(f.y, D.f_range));
  return f;
}
// _apply_action_torque's (core.py:2030-2041); `over`: the norm clamp acted
VD float clamp_torque(const Ent& D, float t, bool& over) {
  over = false;
  if (D.flags & VMAS_F_MAX_T) {
    const float n = fabsf(t);
    const float nt = (t / n) * D.max_t;
    over = n > D.max_t;
    t = over ? nt : t;
  }
  return t;
}
// the velocity clamps of _integrate_state (core.py:2872-2879): v1 behind max_speed, the return value behind v_range
VD v2 clamp_vel(const Ent& D, v2 vpre, v2& v1) {
  v1 = (D.flags & VMAS_F_MAX_SPEED) ? clamp_with_norm(vpre, D.max_speed) : vpre;
  return (D.flags & VMAS_F_V_RANGE) ? V(clamp_t(v1.x, D.v_range), clamp_t(v1.y, D.v_range)) : v1;
}

__global__ void __launch_bounds__(MAX_WAVES * 64)
step_vjp_kernel(const Args A, const float* __restrict__ state_in, const float* __restrict__ ft_in, const long ld,
                const float* __restrict__ g_state_out, const float* __restrict__ g_ft_out, float* __restrict__ g_state_in,
                float* __restrict__ g_ft_in, const int batch) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wv = sgpr((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
  const long env0 = (long)blockIdx.x * ROWF + lane;
  const bool live = env0 < batch;
  const long env = live ? env0 : (long)batch - 1;  // lanes past the batch repeat its last column: they read in bounds, write nothing
  const uint32_t* __restrict__ T = A.tab;
  float* L = lds + lane;  // this lane's column: row r is L[r * ROWF]
  const int S = A.C.substeps, nE = A.nE;
  const float dt = A.C.sub_dt;
  const bool clamp_x = A.C.xs == A.C.xs, clamp_y = A.C.ys == A.C.ys;

  // one pair of a chunk: where its entities' positions of substep s and force-cotangent rows are, and its own two rows
  struct PairRec { int pa, pb, fa, fb; float dist_min; };
  auto load_pair = [&](int p, int s) {
    const uint32_t* Q = T + A.o_pair + p * PW;
    PairRec r;
    r.pa = sgpr((int)Q[0]) + s * sgpr((int)Q[1]);
    r.pb = sgpr((int)Q[2]) + s * sgpr((int)Q[3]);
    r.dist_min = __uint_as_float(Q[4]);
    r.fa = sgpr((int)Q[5]); r.fb = sgpr((int)Q[6]);
    return r;
  };
  auto row2 = [&](int r) { return V(L[r * ROWF], L[(r + 1) * ROWF]); };

  // ---- load: positions into the first checkpoint, velocities, the substep-independent part of the force
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent(T + A.o_ent + e * EW);
    const float* X = state_in + (long)e * 6 * ld + env;
    float* P = L + D.prow * ROWF;
    P[0] = X[0]; P[ROWF] = X[ld];
    if (D.flags & VMAS_F_MOVABLE) {
      float* R = L + D.arow * ROWF;
      R[2 * ROWF] = X[2 * ld]; R[3 * ROWF] = X[3 * ld];
      v2 F = V(0.f, 0.f);
      if (D.flags & VMAS_F_AGENT) {  // _apply_action_force
        const float* Af = ft_in + (long)D.agent_index * 3 * ld + env;
        F = F + clamp_force(D, V(Af[0], Af[ld]));
      }
      if (A.C.has_gravity) F = F + V(D.mass * A.C.gx, D.mass * A.C.gy);  // _apply_gravity core.py:2043-2052
      if (D.flags & VMAS_F_GRAVITY) F = F + V(D.mass * D.gx, D.mass * D.gy);
      R[6 * ROWF] = F.x; R[7 * ROWF] = F.y;
    }
  }
  __syncthreads();

  // ---- forward: the substeps again, checkpointing
  for (int s = 0; s < S; ++s) {
    for (int c = 0; c < A.n_chunks; ++c) {
      const int p0 = c * A.chunk, p1 = min(p0 + A.chunk, A.nP);
      for (int p = p0 + wv; p < p1; p += nw) {
        const PairRec Q = load_pair(p, s);
        const v2 f = contact_force(row2(Q.pa), row2(Q.pb), Q.dist_min, A.C.c_coll, A.C.k);
        float* R = L + (A.row_pairs + 2 * (p - p0)) * ROWF;
        R[0] = f.x; R[ROWF] = f.y;
      }
      __syncthreads();
      for (int e = wv; e < nE; e += nw) {
        const Ent D = load_ent(T + A.o_ent + e * EW);
        if (!(D.flags & VMAS_F_MOVABLE)) continue;
        float* R = L + D.arow * ROWF;
        v2 F = c == 0 ? V(R[6 * ROWF], R[7 * ROWF]) : V(R[0], R[ROWF]);
        const int r0 = sgpr((int)T[A.o_cur + c * nE + e]), r1 = sgpr((int)T[A.o_cur + (c + 1) * nE + e]);
        for (int r = r0; r < r1; ++r) {  // the entity's pairs in the reference's order (core.py:2176-2199): +f on a, -f on b
          const uint32_t rf = (uint32_t)sgpr((int)T[A.o_ref + r]);
          const v2 f = row2(A.row_pairs + 2 * ((int)(rf & 0x7fffffffu) - p0));
          F = (rf >> 31) ? F - f : F + f;
        }
        if (c + 1 < A.n_chunks) { R[0] = F.x; R[ROWF] = F.y; continue; }
        // _integrate_state core.py:2862-2908, as step_kernel does it
        float* K = L + (D.prow + 4 * s) * ROWF;
        v2 vel = V(R[2 * ROWF], R[3 * ROWF]);
        if (s == 0) vel = V(vel.x * D.one_minus_drag, vel.y * D.one_minus_drag);
        const rcp_t rm = rcp_of(D.mass);
        const v2 acc = V(F.x / rm, F.y / rm);
        vel = V(vel.x + acc.x * dt, vel.y + acc.y * dt);
        K[2 * ROWF] = vel.x; K[3 * ROWF] = vel.y;
        v2 v1;
        vel = clamp_vel(D, vel, v1);
        R[2 * ROWF] = vel.x; R[3 * ROWF] = vel.y;
        if (s + 1 < S) {  // (the position behind the last substep is not an input of anything)
          v2 np = V(K[0] + vel.x * dt, K[ROWF] + vel.y * dt);
          if (clamp_x) np.x = clamp_t(np.x, A.C.xs);
          if (clamp_y) np.y = clamp_t(np.y, A.C.ys);
          K[4 * ROWF] = np.x; K[5 * ROWF] = np.y;
        }
      }
      __syncthreads();
    }
  }

  // ---- the cotangents of what the step wrote (rows 0-3 and 6, 7 are their owner's alone: no barrier)
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent(T + A.o_ent + e * EW);
    const float* G = g_state_out + (long)e * 6 * ld + env;
    float* R = L + D.arow * ROWF;
    R[0] = G[0]; R[ROWF] = G[ld];
    if (D.flags & VMAS_F_MOVABLE) {
      R[2 * ROWF] = G[2 * ld]; R[3 * ROWF] = G[3 * ld];
      R[6 * ROWF] = 0.f; R[7 * ROWF] = 0.f;
    }
  }

  // ---- backward sweep
  for (int s = S - 1; s >= 0; --s) {
    for (int e = wv; e < nE; e += nw) {  // the integrator's adjoint
      const Ent D = load_ent(T + A.o_ent + e * EW);
      if (!(D.flags & VMAS_F_MOVABLE)) continue;
      float* R = L + D.arow * ROWF;
      const float* K = L + (D.prow + 4 * s) * ROWF;
      v2 pb = V(R[0], R[ROWF]), vb = V(R[2 * ROWF], R[3 * ROWF]);
      const v2 vpre = V(K[2 * ROWF], K[3 * ROWF]);
      v2 v1;
      const v2 vel = clamp_vel(D, vpre, v1);
      if (clamp_x) pb.x = pass_clamp(K[0] + vel.x * dt, A.C.xs, pb.x);  // position clamps
      if (clamp_y) pb.y = pass_clamp(K[ROWF] + vel.y * dt, A.C.ys, pb.y);
      vb = V(vb.x + pb.x * dt, vb.y + pb.y * dt);                        // pos' = pos + vel' dt
      if (D.flags & VMAS_F_V_RANGE) vb = V(pass_clamp(v1.x, D.v_range, vb.x), pass_clamp(v1.y, D.v_range, vb.y));
      if (D.flags & VMAS_F_MAX_SPEED) vb = clamp_with_norm_vjp(vpre, D.max_speed, vb);
      const rcp_t rm = rcp_of(D.mass);
      const v2 Fb = V((vb.x * dt) / rm, (vb.y * dt) / rm);              // vel' = vel (1 - drag) + F / m dt
      if (s == 0) vb = V(vb.x * D.one_minus_drag, vb.y * D.one_minus_drag);
      R[0] = pb.x; R[ROWF] = pb.y;
      R[2 * ROWF] = vb.x; R[3 * ROWF] = vb.y;
      R[4 * ROWF] = Fb.x; R[5 * ROWF] = Fb.y;
      R[6 * ROWF] += Fb.x; R[7 * ROWF] += Fb.y;
    }
    __syncthreads();
    for (int c = 0; c < A.n_chunks; ++c) {
      const int p0 = c * A.chunk, p1 = min(p0 + A.chunk, A.nP);
      for (int p = p0 + wv; p < p1; p += nw) {  // the pair adjoint: fbar = Fbar_a - Fbar_b over the movable ends
        const PairRec Q = load_pair(p, s);
        v2 fb = V(0.f, 0.f);
        if (Q.fa >= 0) fb = row2(Q.fa);
        if (Q.fb >= 0) fb = fb - row2(Q.fb);
        const v2 db = contact_force_vjp(row2(Q.pa), row2(Q.pb), Q.dist_min, A.C.c_coll, A.C.k, fb);
        float* R = L + (A.row_pairs + 2 * (p - p0)) * ROWF;
        R[0] = db.x; R[ROWF] = db.y;
      }
      __syncthreads();
      for (int e = wv; e < nE; e += nw) {  // position cotangents go to both ends, movable or not
        const int r0 = sgpr((int)T[A.o_cur + c * nE + e]), r1 = sgpr((int)T[A.o_cur + (c + 1) * nE + e]);
        if (r0 == r1) continue;
        float* R = L + sgpr((int)T[A.o_ent + e * EW + 2]) * ROWF;
        v2 pb = V(R[0], R[ROWF]);
        for (int r = r0; r < r1; ++r) {
          const uint32_t rf = (uint32_t)sgpr((int)T[A.o_ref + r]);
          const v2 db = row2(A.row_pairs + 2 * ((int)(rf & 0x7fffffffu) - p0));
          pb = (rf >> 31) ? pb - db : pb + db;
        }
        R[0] = pb.x; R[ROWF] = pb.y;
      }
      __syncthreads();
    }
  }

  // ---- out: state cotangents (rotation in closed form), then the force cotangents pulled back through the action clamps
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent(T + A.o_ent + e * EW);
    const float* G = g_state_out + (long)e * 6 * ld + env;
    const float* R = L + D.arow * ROWF;
    const bool mov = D.flags & VMAS_F_MOVABLE, rotb = D.flags & VMAS_F_ROTATABLE;
    const v2 vb = mov ? V(R[2 * ROWF], R[3 * ROWF]) : V(G[2 * ld], G[3 * ld]);
    float rb = G[4 * ld], ab = G[5 * ld], Tb = 0.f;
    if (rotb)  // ang_vel' = ang_vel (1 - drag on substep 0) + Tq / I dt, rot' = rot + ang_vel' dt
      for (int s = S - 1; s >= 0; --s) {
        ab = ab + rb * dt;
        Tb = Tb + (ab * dt) / D.inertia;
        if (s == 0) ab = ab * D.one_minus_drag;
      }
    if (live) {
      float* O = g_state_in + (long)e * 6 * ld + env0;
      O[0] = R[0]; O[ld] = R[ROWF]; O[2 * ld] = vb.x; O[3 * ld] = vb.y; O[4 * ld] = rb; O[5 * ld] = ab;
    }
    if (!(D.flags & VMAS_F_AGENT)) continue;
    const long ao = (long)D.agent_index * 3 * ld;
    v2 fb = V(0.f, 0.f);
    float tb = 0.f;
    if (g_ft_out != nullptr) { fb = V(g_ft_out[ao + env], g_ft_out[ao + ld + env]); tb = g_ft_out[ao + 2 * ld + env]; }
    if (mov) {  // (an agent that cannot move keeps its force untouched: the cotangent passes)
      fb = fb + V(R[6 * ROWF], R[7 * ROWF]);
      const v2 raw = V(ft_in[ao + env], ft_in[ao + ld + env]);
      if (D.flags & VMAS_F_F_RANGE) {
        const v2 f1 = (D.flags & VMAS_F_MAX_F) ? clamp_with_norm(raw, D.max_f) : raw;
        fb = V(pass_clamp(f1.x, D.f_range, fb.x), pass_clamp(f1.y, D.f_range, fb.y));
      }
      if (D.flags & VMAS_F_MAX_F) fb = clamp_with_norm_vjp(raw, D.max_f, fb);
    }
    if (rotb) {
      tb = tb + Tb;
      bool over;
      const float t1 = clamp_torque(D, ft_in[ao + 2 * ld + env], over);
      if (D.flags & VMAS_F_T_RANGE) tb = pass_clamp(t1, D.t_range, tb);
      tb = over ? 0.f : tb;  // t / |t| max_t does not depend on |t|
    }
    if (live) { g_ft_in[ao + env0] = fb.x; g_ft_in[ao + ld + env0] = fb.y; g_ft_in[ao + 2 * ld + env0] = tb; }
  }
}

uint32_t fbits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

}  // namespace

void make_plan(const WorldConst& C, const VmasEntityDesc* ents, int nE, int nA, const VmasPairDesc* pairs, int nP_all,
               int n_joints, Plan* out) {
  Plan& P = *out;
  P = Plan{};
  P.C = C; P.nE = nE; P.nA = nA;
  auto refuse = [&](const char* fmt, auto... a) { snprintf(P.why, sizeof(P.why), fmt, a...); };
  for (int p = 0; p < nP_all; ++p)
    if (pairs[p].type != VMAS_PAIR_SS)
      return refuse("pair %d (entities %d, %d) has type %d, the backward kernel serves sphere-sphere pairs only (lines and boxes "
                    "are out of its scope)", p, pairs[p].a, pairs[p].b, pairs[p].type);
  if (n_joints > 0) return refuse("the world has %d joint constraint(s), which the backward kernel does not serve", n_joints);
  for (int e = 0; e < nE; ++e)
    if (ents[e].flags & (VMAS_F_LIN_FRICTION | VMAS_F_ANG_FRICTION))
      return refuse("entity %d has %s friction, which the backward kernel does not serve", e,
                    (ents[e].flags & VMAS_F_LIN_FRICTION) ? "linear" : "angular");
  // tile rows
  std::vector<int> arow(nE), prow(nE);
  int rows = 0, n_mov = 0;
  for (int e = 0; e < nE; ++e) {
    const bool mov = ents[e].flags & VMAS_F_MOVABLE;
    arow[e] = rows;
    prow[e] = rows + (mov ? 8 : 2);
    rows += mov ? 8 + 4 * C.substeps : 4;
    n_mov += mov;
  }
  // pairs without a movable end exert no force on anything and get no cotangent: left out
  std::vector<int> kept;
  for (int p = 0; p < nP_all; ++p)
    if ((ents[pairs[p].a].flags | ents[pairs[p].b].flags) & VMAS_F_MOVABLE) kept.push_back(p);
  P.nP = (int)kept.size();
  const size_t ent_bytes = (size_t)rows * ROWF * sizeof(float), pair_bytes = 2 * ROWF * sizeof(float);
  const int want = P.nP < MAX_WAVES ? P.nP : MAX_WAVES;  // a run of fewer pairs than waves would idle most of the block
  if (ent_bytes + want * pair_bytes > kLdsMax)
    return refuse("a 64-environment tile needs %zu B of LDS for the adjoint and checkpoint rows of %d entities over %d substeps "
                  "and %zu B for the rows of %d pairs, the compute unit has %zu B", ent_bytes, nE, C.substeps,
                  want * pair_bytes, want, kLdsMax);
  const int fit = (int)((kLdsMax - ent_bytes) / pair_bytes);
  P.n_chunks = P.nP > 0 ? (P.nP + fit - 1) / fit : 1;
  P.chunk = (P.nP + P.n_chunks - 1) / P.n_chunks;
  P.row_pairs = rows;
  P.n_rows = rows + 2 * P.chunk;
  P.lds_bytes = (size_t)P.n_rows * ROWF * sizeof(float);
  const int work = n_mov > P.chunk ? n_mov : P.chunk;
  P.nw = work < 1 ? 1 : (work > MAX_WAVES ? MAX_WAVES : work);
  // the table
  std::vector<uint32_t>& T = P.table;
  P.o_ent = 0;
  T.assign((size_t)nE * EW, 0u);
  for (int e = 0; e < nE; ++e) {
    const VmasEntityDesc& s = ents[e];
    uint32_t* w = &T[(size_t)e * EW];
    w[0] = s.flags; w[1] = (uint32_t)s.agent_index; w[2] = (uint32_t)arow[e]; w[3] = (uint32_t)prow[e];
    w[5] = fbits(s.mass); w[6] = fbits(s.inertia); w[7] = fbits(s.one_minus_drag);
    w[8] = fbits(s.max_speed); w[9] = fbits(s.v_range); w[10] = fbits(s.gravity[0]); w[11] = fbits(s.gravity[1]);
    w[12] = fbits(s.max_f); w[13] = fbits(s.f_range); w[14] = fbits(s.max_t); w[15] = fbits(s.t_range);
  }
  P.o_pair = (int)T.size();
  for (int p : kept) {
    const int a = pairs[p].a, b = pairs[p].b;
    const bool ma = ents[a].flags & VMAS_F_MOVABLE, mb = ents[b].flags & VMAS_F_MOVABLE;
    const uint32_t w[PW] = {(uint32_t)prow[a], ma ? 4u : 0u, (uint32_t)prow[b], mb ? 4u : 0u,
                            fbits(ents[a].radius + ents[b].radius),  // (fp32 sum, as the forward's items carry it)
                            (uint32_t)(ma ? arow[a] + 4 : -1), (uint32_t)(mb ? arow[b] + 4 : -1), 0u};
    T.insert(T.end(), w, w + PW);
  }
  // per entity its pairs in pair order (index | side << 31), and where each chunk's run of them starts
  P.o_ref = (int)T.size();
  std::vector<int> ref_begin(nE + 1, 0);
  for (int e = 0; e < nE; ++e) {
    ref_begin[e] = (int)T.size() - P.o_ref;
    for (int i = 0; i < P.nP; ++i) {
      if (pairs[kept[i]].a == e) T.push_back((uint32_t)i);
      else if (pairs[kept[i]].b == e) T.push_back((uint32_t)i | 0x80000000u);
    }
  }
  ref_begin[nE] = (int)T.size() - P.o_ref;
  P.o_cur = (int)T.size();
  for (int c = 0; c <= P.n_chunks; ++c)
    for (int e = 0; e < nE; ++e) {
      int r = ref_begin[e];
      while (r < ref_begin[e + 1] && (int)(T[P.o_ref + r] & 0x7fffffffu) < c * P.chunk) ++r;
      T.push_back((uint32_t)(c == P.n_chunks ? ref_begin[e + 1] : r));
    }
  P.ok = true;
}

int upload(Plan* p) {
  if (hipMalloc((void**)&p->d_table, p->table.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(p->d_table, p->table.data(), p->table.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    return host_fail("vmas_world_create: uploading the backward kernel's table failed");
  return 0;
}

void release(Plan* p) {
  if (p->d_table) (void)hipFree(p->d_table);
  p->d_table = nullptr;
}

int launch(const Plan& p, int device, int batch, const float* state_in, const float* ft_in, long ld, const float* g_state_out,
           const float* g_ft_out, float* g_state_in, float* g_ft_in, hipStream_t s) {
  if (!p.ok || !p.d_table) return host_fail("vmas_world_step_vjp: the world has no backward plan");
  if (p.lds_bytes > 64 * 1024) {  // opt in to the large LDS once per device
    static std::atomic<size_t> set_for_dev[64];
    std::atomic<size_t>& set_for = set_for_dev[device & 63];
    if (set_for.load() < p.lds_bytes) {
      if (hipFuncSetAttribute((const void*)step_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess)
        return host_fail("vmas_world_step_vjp: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      set_for = kLdsMax;
    }
  }
  Args A;
  A.C = p.C;
  A.nE = p.nE; A.nP = p.nP; A.chunk = p.chunk; A.n_chunks = p.n_chunks; A.row_pairs = p.row_pairs;
  A.o_ent = p.o_ent; A.o_pair = p.o_pair; A.o_ref = p.o_ref; A.o_cur = p.o_cur;
  A.tab = p.d_table;
  const dim3 grid((batch + ROWF - 1) / ROWF), block(ROWF * p.nw);
  hipLaunchKernelGGL(step_vjp_kernel, grid, block, p.lds_bytes, s, A, state_in, ft_in, ld, g_state_out, g_ft_out, g_state_in,
                     g_ft_in, batch);
  if (hipGetLastError() != hipSuccess) return host_fail("vmas_world_step_vjp: launch of the backward kernel failed");
  return 0;
}

}  // namespace vjp
}  // namespace vmas
