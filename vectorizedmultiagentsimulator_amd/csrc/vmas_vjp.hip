// vmas_vjp.hip - the backward kernel of World.step for worlds of sphere-sphere, line-sphere and box-sphere pairs: one
// launch computes the vector-Jacobian product of one vmas_world_step (include/vmas_hip.h, vmas_world_step_vjp; DESIGN.md
// "Backward of World.step").
//
// Lane = environment, a block owns a tile of 64 environments, as the forward does.  The launch
//   1. re-runs the step's substeps from the saved pre-step state with the forward's own device functions (contact_force,
//      clamp_action_force / _torque, accelerate, clamp_velocity, integrate_position / _rotation: vmas_device.h), so every
//      clamp and contact decision has the forward's bits, and
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
// Rotation of an entity that is no line or box of a served pair needs no checkpoint: rot and ang_vel are linear in the
// (once clamped) torque, their adjoint over all substeps is a closed form evaluated by the entity's owner on its way out.
// A line or box that is `a` of a line-sphere / box-sphere pair ("shaped" below) has a block of rows of its own: contacts
// exert torque on it and the contact point depends on its rotation, so its rotation is integrated per substep, rot is
// checkpointed per substep (one row, when it can rotate) and cos/sin of it are kept in rows the pairs read.  Worlds without
// such a pair run the instantiation without any of that code (step_vjp_kernel<false>).
//
// Tile rows (64 floats each), per entity e at row arow(e):
//   movable:    0,1  forward: force sum carried between chunks   backward: position cotangent
//               2,3  forward: velocity                           backward: velocity cotangent
//               4,5                                              backward: this substep's force cotangent (read by the pairs)
//               6,7  forward: action force (clamped) + gravity   backward: force cotangent summed over the substeps
//               8 + 4 s ...: checkpoint of substep s: pos.x pos.y, pre-clamp vel.x vel.y
//   immovable:  0,1  position cotangent;  2,3  position
//   shaped, at row qrow(e):
//               0    backward: rot cotangent
//               1    forward: ang_vel                            backward: ang_vel cotangent
//               2    forward: torque sum carried between chunks  backward: this substep's torque cotangent (read by the pairs)
//               3    forward: action torque (clamped)            backward: torque cotangent summed over the substeps
//               4 ...: cos, sin of rot (a box: and of rot + pi/2) of the substep at hand
//               then rot at the input of substep s (one row per substep if the entity can rotate, else one row)
// then the rows of a chunk's pairs: 2 per sphere-sphere pair (forward: the force on a; backward: dbar), 5 per line-sphere /
// box-sphere pair (forward: the force on a and the torque on a; backward: pa_bar, pb_bar, rot_bar of a).
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

constexpr int ROWF = kRow;               // floats per LDS row = environments per tile
constexpr int EW = 20, PW = 14;          // table words per entity / per pair
constexpr int SS_ROWS = 2, SHAPE_ROWS = 5;  // LDS rows of a sphere-sphere pair / of a line-sphere or box-sphere pair
// an owner's reference to a pair: index | the pair's first row in its chunk << 16 | shaped << 30 | side << 31
constexpr uint32_t REF_IDX = 0xffffu, REF_ROW = 0x3fffu, REF_SHAPED = 1u << 30;
constexpr int REF_ROW_SHIFT = 16;
constexpr uint32_t PT_HOLLOW = 1u << 8;  // word 7 of a pair record: VMAS_PAIR_* | PT_HOLLOW
constexpr int MAX_WAVES = 8;
constexpr size_t kLdsMax = 160 * 1024;   // LDS of one gfx950 CU

struct Args {
  WorldConst C;
  int32_t nE, n_chunks, row_pairs;
  int32_t o_ent, o_pair, o_ref, o_cur, o_chk;
  const uint32_t* tab;
};

VD int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct Ent {
  uint32_t flags; int32_t agent_index, arow, prow, qrow, nt;  // wave-uniform (qrow < 0: not shaped; nt: trig rows)
  float mass, inertia, one_minus_drag, max_speed, v_range, gx, gy, max_f, f_range, max_t, t_range;
};
template <bool SH>  // (without shaped entities their words are not even fetched)
VD Ent load_ent(const uint32_t* p) {
  Ent D;
  D.flags = (uint32_t)sgpr((int)p[0]); D.agent_index = sgpr((int)p[1]); D.arow = sgpr((int)p[2]); D.prow = sgpr((int)p[3]);
  D.qrow = -1; D.nt = 0;
  if constexpr (SH) { D.qrow = sgpr((int)p[4]); D.nt = sgpr((int)p[16]); }
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

// The same for a line-sphere / box-sphere contact, whose cotangent of the force depends on the force itself (the torque's
// lever) and whose dist_min may depend on the state (a solid box: + depth): the coefficients once, then
//   force      f = c g d
//   dbar         = c (g fb + (g' / dist) (d . fb) d)
//   dist_minbar  = c (d . fb) / dist * sigmoid(x)
// `on` false: the forward zeroes the force (every coefficient is 0 then).
struct ContactTerms { v2 d; float cg, cs, cm; bool any; };
VD ContactTerms contact_terms(v2 pa, v2 pb, float dist_min, float c, float k) {
  ContactTerms t;
  t.d = pa - pb;
  t.cg = t.cs = t.cm = 0.f;
  const float dist = vnorm(t.d);
  t.any = __any(!(dist > dist_min));
  if (!t.any) return t;
  const float x = (dist_min - dist) / rcp_of(k);
  const float pen = softplus0(x) * k;
  const rcp_t den = rcp_of(dist > 0.f ? dist : 1e-8f);
  const float sig = 1.f / rcp_of(1.f + expf(0.f - x));
  const float g = pen / den;
  const float gp = ((0.f - sig) - g) / den;
  const bool zero = (dist < 1e-6f) || (dist > dist_min);
  t.cg = zero ? 0.f : c * g;
  t.cs = zero ? 0.f : c * (gp / den);
  t.cm = zero ? 0.f : c * (sig / den);
  return t;
}

// VJP of closest_point_line<true>(pos, c, s, half, p) (vmas_device.h) for the cotangent cpb of the point: cp = pos - t u,
// t = clamp(dot, +-half), dot = (pos - p) . u, u = (c, s).  -> cotangents of pos, of p and of u.
struct LineAdj { v2 posb, pb, ub; };
VD LineAdj closest_point_line_vjp(v2 pos, float c, float s, float half, v2 p, v2 cpb) {
  const v2 d = pos - p;
  const float dot = d.x * c + d.y * s;
  const float t = clamp_t(dot, half);
  const float tb = 0.f - (cpb.x * c + cpb.y * s);
  const float dotb = pass_clamp(dot, half, tb);
  LineAdj r;
  r.posb = V(cpb.x + dotb * c, cpb.y + dotb * s);
  r.pb = V(0.f - dotb * c, 0.f - dotb * s);
  r.ub = V(dotb * d.x - t * cpb.x, dotb * d.y - t * cpb.y);
  return r;
}

// What a line-sphere / box-sphere pair gives back: the cotangents of the line's or box's position, of the sphere's
// position and of the line's or box's rotation.
struct ShapeAdj { v2 pab, pbb; float rotb; };

// Adjoint of the contact shared by both pair types.  The sphere at pb is pushed away from the point q (the closest point
// of the line, the surface or the inner point of the box) with F = contact_force(pb, q, dist_min); the line or box gets
// -F and the torque cross(cp - pa, -F).  Fa, Fb, Ta: cotangents of the force on a, on b and of the torque on a.
//   -> dbar (cotangent of pb - q), the lever's cotangent rbar and dist_min's cotangent
VD void contact_adjoint(const ContactTerms& K, v2 lever, v2 Fa, v2 Fb, float Ta, v2& db, v2& rb, float& dminb) {
  const v2 F = V(K.cg * K.d.x, K.cg * K.d.y);
  const v2 fb = V((Fb.x - Fa.x) + Ta * lever.y, (Fb.y - Fa.y) - Ta * lever.x);  // torque on a = -(lever x F)
  rb = V(0.f - Ta * F.y, Ta * F.x);
  const float df = vdot(K.d, fb);
  db = V(K.cg * fb.x + (K.cs * df) * K.d.x, K.cg * fb.y + (K.cs * df) * K.d.y);
  dminb = K.cm * df;
}

// a = line (centre pa, cos/sin c, s, half length), b = sphere: core.py:2341-2392 as eval_item evaluates it
VD ShapeAdj line_sphere_vjp(v2 pa, float c, float s, float half, v2 pb, float dist_min, float cc, float k, v2 Fa, v2 Fb,
                            float Ta) {
  ShapeAdj R;
  R.pab = V(0.f, 0.f); R.pbb = V(0.f, 0.f); R.rotb = 0.f;
  const v2 cp = closest_point_line<true>(pa, c, s, half, pb);
  const ContactTerms K = contact_terms(pb, cp, dist_min, cc, k);
  if (!K.any) return R;
  v2 db, rb;
  float dminb;
  contact_adjoint(K, cp - pa, Fa, Fb, Ta, db, rb, dminb);
  const v2 cpb = rb - db;
  const LineAdj A = closest_point_line_vjp(pa, c, s, half, pb, cpb);
  R.pab = A.posb - rb;
  R.pbb = db + A.pb;
  R.rotb = A.ub.y * c - A.ub.x * s;  // d (cos, sin) / d rot = (-sin, cos)
  return R;
}

// a = box (centre pa, cos/sin of rot and of rot + pi/2, length, width, hollow or solid), b = sphere: core.py:2459-2552
VD ShapeAdj box_sphere_vjp(v2 pa, float c, float s, float c2, float s2, float length, float width, bool hollow, v2 pb,
                           float dist_min, float cc, float k, v2 Fa, v2 Fb, float Ta) {
  ShapeAdj R;
  R.pab = V(0.f, 0.f); R.pbb = V(0.f, 0.f); R.rotb = 0.f;
  seg_t be[4];
  box_edges(pa, c, s, c2, s2, length, width, be);
  int edge;
  const v2 cp = closest_point_box(be, pb, edge);
  v2 ip = cp;
  float depth = 0.f;
  if (!hollow) ip = inner_point_box(pb, cp, pa, depth);
  const ContactTerms K = contact_terms(pb, ip, dist_min + depth, cc, k);
  if (!K.any) return R;
  v2 db, rb;
  float dminb;
  contact_adjoint(K, cp - pa, Fa, Fb, Ta, db, rb, dminb);
  v2 pab = V(0.f - rb.x, 0.f - rb.y), pbb = db;
  v2 cpb = rb - db;  // the lever, and the inner point where it is the surface point
  if (!hollow) {     // inner_point_box: ip = cp + vh xm, xm = vh . (pa - cp), vh = (cp - pb) / n, depth = |xm|
    const v2 v = cp - pb, u = pa - cp;
    const float n = vnorm(v);
    const bool z = n == 0.f;  // (the forward takes the surface point and depth 0 there)
    const rcp_t rn = rcp_of(z ? 1.f : n);
    const v2 vh = V(v.x / rn, v.y / rn);
    const float xm = vdot(vh, u);
    const v2 ipb = V(0.f - db.x, 0.f - db.y);
    const float xmb = vdot(ipb, vh) + sign_t(xm) * dminb;
    const v2 vhb = V(xm * ipb.x + xmb * u.x, xm * ipb.y + xmb * u.y);
    const float along = vdot(vh, vhb);
    const v2 vb = V((vhb.x - vh.x * along) / rn, (vhb.y - vh.y * along) / rn);
    const v2 ub = V(xmb * vh.x, xmb * vh.y);
    cpb = cpb + (z ? V(0.f, 0.f) : vb - ub);
    pbb = pbb - (z ? V(0.f, 0.f) : vb);
    pab = pab + (z ? V(0.f, 0.f) : ub);
  }
  // the winning edge (physics.py:298-325): edges 0, 1 sit at +-L/2 along (c, s) and run along (c2, s2), edges 2, 3 at
  // +-W/2 along (c2, s2) and run along (c, s)
  const bool along_box = edge >= 2;
  const v2 epos = edge == 0 ? be[0].pos : edge == 1 ? be[1].pos : edge == 2 ? be[2].pos : be[3].pos;
  const float ec = along_box ? c : c2, es = along_box ? s : s2, eh = along_box ? be[2].half : be[0].half;
  const float oc = along_box ? c2 : c, os = along_box ? s2 : s;  // the axis the edge's centre is offset along
  const float off = along_box ? be[0].half : be[2].half;          // (be[0].half = W/2, be[2].half = L/2)
  const float reach = (edge & 1) ? 0.f - off : off;
  const LineAdj A = closest_point_line_vjp(epos, ec, es, eh, pb, cpb);
  R.pab = pab + A.posb;
  R.pbb = pbb + A.pb;
  const v2 ob = V(reach * A.posb.x, reach * A.posb.y);  // centre = pa + reach (oc, os)
  R.rotb = (A.ub.y * ec - A.ub.x * es) + (ob.y * oc - ob.x * os);
  return R;
}

// SH: the world has line-sphere / box-sphere pairs.  Without them none of their code is in the kernel.
template <bool SH>
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

  // one pair of a chunk: where its entities' positions of substep s and force-cotangent rows are, and its own rows; a
  // line-sphere / box-sphere pair also: its type, a's trig rows and torque-cotangent row, a's dimensions
  struct PairRec { int pa, pb, fa, fb, row, type, tr, ta; float dist_min, p0, p1; };
  auto load_pair = [&](int p, int p0, int s) {
    const uint32_t* Q = T + A.o_pair + p * PW;
    PairRec r;
    r.pa = sgpr((int)Q[0]) + s * sgpr((int)Q[1]);
    r.pb = sgpr((int)Q[2]) + s * sgpr((int)Q[3]);
    r.dist_min = __uint_as_float(Q[4]);
    r.fa = sgpr((int)Q[5]); r.fb = sgpr((int)Q[6]);
    r.row = A.row_pairs + (SH ? sgpr((int)Q[8]) : SS_ROWS * (p - p0));
    r.type = VMAS_PAIR_SS; r.tr = 0; r.ta = -1; r.p0 = r.p1 = 0.f;
    if constexpr (SH) {
      r.type = sgpr((int)Q[7]); r.tr = sgpr((int)Q[9]); r.ta = sgpr((int)Q[10]);
      r.p0 = __uint_as_float(Q[11]); r.p1 = __uint_as_float(Q[12]);
    }
    return r;
  };
  auto row2 = [&](int r) { return V(L[r * ROWF], L[(r + 1) * ROWF]); };
  auto chunk_begin = [&](int c) { return sgpr((int)T[A.o_chk + c]); };

  // ---- load: positions into the first checkpoint, velocities, the substep-independent part of the force
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent<SH>(T + A.o_ent + e * EW);
    const float* X = state_in + (long)e * 6 * ld + env;
    float* P = L + D.prow * ROWF;
    P[0] = X[0]; P[ROWF] = X[ld];
    if (SH && D.qrow >= 0) {  // rot into its first checkpoint and its cos/sin, ang_vel, the action torque
      float* Q = L + D.qrow * ROWF;
      const float rot = X[4 * ld];
      Q[(4 + D.nt) * ROWF] = rot;
      write_trig(Q + 4 * ROWF, rot, D.nt);
      Q[1 * ROWF] = X[5 * ld];
      float Tq = 0.f;
      if ((D.flags & VMAS_F_AGENT) && (D.flags & VMAS_F_ROTATABLE))  // _apply_action_torque
        Tq = Tq + clamp_action_torque(ft_in[((long)D.agent_index * 3 + 2) * ld + env], D.flags & VMAS_F_MAX_T, D.max_t,
                                      D.flags & VMAS_F_T_RANGE, D.t_range).t;
      Q[3 * ROWF] = Tq;
    }
    if (D.flags & VMAS_F_MOVABLE) {
      float* R = L + D.arow * ROWF;
      R[2 * ROWF] = X[2 * ld]; R[3 * ROWF] = X[3 * ld];
      v2 F = V(0.f, 0.f);
      if (D.flags & VMAS_F_AGENT) {  // _apply_action_force
        const float* Af = ft_in + (long)D.agent_index * 3 * ld + env;
        F = F + clamp_action_force(V(Af[0], Af[ld]), D.flags & VMAS_F_MAX_F, D.max_f, D.flags & VMAS_F_F_RANGE, D.f_range).f;
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
      const int p0 = chunk_begin(c), p1 = chunk_begin(c + 1);
      for (int p = p0 + wv; p < p1; p += nw) {
        const PairRec Q = load_pair(p, p0, s);
        float* R = L + Q.row * ROWF;
        const v2 pa = row2(Q.pa), pb = row2(Q.pb);
        if (!SH || Q.type == VMAS_PAIR_SS) {
          const v2 f = contact_force(pa, pb, Q.dist_min, A.C.c_coll, A.C.k);
          R[0] = f.x; R[ROWF] = f.y;
        } else {  // a = line or box, b = sphere, as eval_item evaluates them (vmas_step_device.h): the force on a and its torque
          const float* TA = L + Q.tr * ROWF;
          v2 cp, f;
          if ((Q.type & 0xff) == VMAS_PAIR_LS) {
            cp = closest_point_line<true>(pa, TA[0], TA[ROWF], Q.p0, pb);
            f = -contact_force(pb, cp, Q.dist_min, A.C.c_coll, A.C.k);
          } else {
            seg_t be[4];
            box_edges(pa, TA[0], TA[ROWF], TA[2 * ROWF], TA[3 * ROWF], Q.p0, Q.p1, be);
            cp = closest_point_box(be, pb);
            v2 ip = cp;
            float d = 0.f;
            if (!(Q.type & PT_HOLLOW)) ip = inner_point_box(pb, cp, pa, d);
            f = -contact_force(pb, ip, Q.dist_min + d, A.C.c_coll, A.C.k);
          }
          R[0] = f.x; R[ROWF] = f.y; R[2 * ROWF] = vcross(cp - pa, f);
        }
      }
      __syncthreads();
      for (int e = wv; e < nE; e += nw) {
        const Ent D = load_ent<SH>(T + A.o_ent + e * EW);
        const bool mov = D.flags & VMAS_F_MOVABLE, turns = SH && D.qrow >= 0 && (D.flags & VMAS_F_ROTATABLE);
        if (!mov && !turns) continue;
        float* R = L + D.arow * ROWF;
        float* Qr = L + (turns ? D.qrow : 0) * ROWF;
        v2 F = V(0.f, 0.f);
        float Tq = 0.f;
        if (mov) F = c == 0 ? V(R[6 * ROWF], R[7 * ROWF]) : V(R[0], R[ROWF]);
        if (turns) Tq = c == 0 ? Qr[3 * ROWF] : Qr[2 * ROWF];
        const int r0 = sgpr((int)T[A.o_cur + c * nE + e]), r1 = sgpr((int)T[A.o_cur + (c + 1) * nE + e]);
        for (int r = r0; r < r1; ++r) {  // the entity's pairs in the reference's order (core.py:2176-2199): +f on a, -f on b
          const uint32_t rf = (uint32_t)sgpr((int)T[A.o_ref + r]);
          const int row = A.row_pairs + (int)((rf >> REF_ROW_SHIFT) & REF_ROW);
          const v2 f = row2(row);
          if (mov) F = (rf >> 31) ? F - f : F + f;
          if (turns && (rf & REF_SHAPED) && !(rf >> 31)) Tq = Tq + L[(row + 2) * ROWF];
        }
        if (c + 1 < A.n_chunks) {
          if (mov) { R[0] = F.x; R[ROWF] = F.y; }
          if (turns) Qr[2 * ROWF] = Tq;
          continue;
        }
        if (turns) {
          const rotation_t rt = integrate_rotation(Qr[(4 + D.nt + s) * ROWF], Qr[1 * ROWF], Tq, D.inertia, D.one_minus_drag, s == 0, dt);
          Qr[1 * ROWF] = rt.av;
          if (s + 1 < S) {
            Qr[(4 + D.nt + s + 1) * ROWF] = rt.rot;
            write_trig(Qr + 4 * ROWF, rt.rot, D.nt);
          }
        }
        if (!mov) continue;
        float* K = L + (D.prow + 4 * s) * ROWF;
        const v2 pre = accelerate(V(R[2 * ROWF], R[3 * ROWF]), F, D.mass, D.one_minus_drag, s == 0, dt);
        K[2 * ROWF] = pre.x; K[3 * ROWF] = pre.y;
        const v2 vel = clamp_velocity(pre, D.flags & VMAS_F_MAX_SPEED, D.max_speed, D.flags & VMAS_F_V_RANGE, D.v_range).v;
        R[2 * ROWF] = vel.x; R[3 * ROWF] = vel.y;
        if (s + 1 < S) {  // (the position behind the last substep is not an input of anything)
          const v2 np = integrate_position(V(K[0], K[ROWF]), vel, dt, A.C.xs, A.C.ys).p;
          K[4 * ROWF] = np.x; K[5 * ROWF] = np.y;
        }
      }
      __syncthreads();
    }
  }

  // ---- the cotangents of what the step wrote (rows 0-3 and 6, 7 are their owner's alone: no barrier)
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent<SH>(T + A.o_ent + e * EW);
    const float* G = g_state_out + (long)e * 6 * ld + env;
    float* R = L + D.arow * ROWF;
    R[0] = G[0]; R[ROWF] = G[ld];
    if (D.flags & VMAS_F_MOVABLE) {
      R[2 * ROWF] = G[2 * ld]; R[3 * ROWF] = G[3 * ld];
      R[6 * ROWF] = 0.f; R[7 * ROWF] = 0.f;
    }
    if (SH && D.qrow >= 0) {
      float* Q = L + D.qrow * ROWF;
      Q[0] = G[4 * ld]; Q[1 * ROWF] = G[5 * ld]; Q[3 * ROWF] = 0.f;
    }
  }

  // ---- backward sweep
  for (int s = S - 1; s >= 0; --s) {
    for (int e = wv; e < nE; e += nw) {  // the integrator's adjoint
      const Ent D = load_ent<SH>(T + A.o_ent + e * EW);
      if (SH && D.qrow >= 0 && (D.flags & VMAS_F_ROTATABLE)) {
        float* Q = L + D.qrow * ROWF;
        const float ab = Q[1 * ROWF] + Q[0] * dt;      // rot' = rot + ang_vel' dt
        const float Tb = (ab * dt) / D.inertia;        // ang_vel' = ang_vel (1 - drag) + Tq / I dt
        Q[1 * ROWF] = s == 0 ? ab * D.one_minus_drag : ab;
        Q[2 * ROWF] = Tb;
        Q[3 * ROWF] += Tb;
        if (s + 1 < S) write_trig(Q + 4 * ROWF, Q[(4 + D.nt + s) * ROWF], D.nt);  // this substep's cos/sin again (the last one's are still there)
      }
      if (!(D.flags & VMAS_F_MOVABLE)) continue;
      float* R = L + D.arow * ROWF;
      const float* K = L + (D.prow + 4 * s) * ROWF;
      v2 pb = V(R[0], R[ROWF]), vb = V(R[2 * ROWF], R[3 * ROWF]);
      const v2 pre = V(K[2 * ROWF], K[3 * ROWF]);
      const velocity_t v = clamp_velocity(pre, D.flags & VMAS_F_MAX_SPEED, D.max_speed, D.flags & VMAS_F_V_RANGE, D.v_range);
      if (clamp_x || clamp_y) {  // position clamps
        const v2 np = integrate_position(V(K[0], K[ROWF]), v.v, dt, A.C.xs, A.C.ys).raw;
        if (clamp_x) pb.x = pass_clamp(np.x, A.C.xs, pb.x);
        if (clamp_y) pb.y = pass_clamp(np.y, A.C.ys, pb.y);
      }
      vb = V(vb.x + pb.x * dt, vb.y + pb.y * dt);  // pos' = pos + vel' dt
      if (D.flags & VMAS_F_V_RANGE) vb = V(pass_clamp(v.v1.x, D.v_range, vb.x), pass_clamp(v.v1.y, D.v_range, vb.y));
      if (D.flags & VMAS_F_MAX_SPEED) vb = clamp_with_norm_vjp(pre, D.max_speed, vb);
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
      const int p0 = chunk_begin(c), p1 = chunk_begin(c + 1);
      for (int p = p0 + wv; p < p1; p += nw) {  // the pair adjoint: fbar = Fbar_a - Fbar_b over the movable ends
        const PairRec Q = load_pair(p, p0, s);
        float* R = L + Q.row * ROWF;
        if (!SH || Q.type == VMAS_PAIR_SS) {
          v2 fb = V(0.f, 0.f);
          if (Q.fa >= 0) fb = row2(Q.fa);
          if (Q.fb >= 0) fb = fb - row2(Q.fb);
          const v2 db = contact_force_vjp(row2(Q.pa), row2(Q.pb), Q.dist_min, A.C.c_coll, A.C.k, fb);
          R[0] = db.x; R[ROWF] = db.y;
        } else {  // line-sphere / box-sphere: the cotangents of a's position, b's position and a's rotation
          const v2 Fa = Q.fa >= 0 ? row2(Q.fa) : V(0.f, 0.f), Fb = Q.fb >= 0 ? row2(Q.fb) : V(0.f, 0.f);
          const float Ta = Q.ta >= 0 ? L[Q.ta * ROWF] : 0.f;
          const float* TA = L + Q.tr * ROWF;
          ShapeAdj G;
          if ((Q.type & 0xff) == VMAS_PAIR_LS)
            G = line_sphere_vjp(row2(Q.pa), TA[0], TA[ROWF], Q.p0, row2(Q.pb), Q.dist_min, A.C.c_coll, A.C.k, Fa, Fb, Ta);
          else
            G = box_sphere_vjp(row2(Q.pa), TA[0], TA[ROWF], TA[2 * ROWF], TA[3 * ROWF], Q.p0, Q.p1, (Q.type & PT_HOLLOW) != 0,
                               row2(Q.pb), Q.dist_min, A.C.c_coll, A.C.k, Fa, Fb, Ta);
          R[0] = G.pab.x; R[ROWF] = G.pab.y; R[2 * ROWF] = G.pbb.x; R[3 * ROWF] = G.pbb.y; R[4 * ROWF] = G.rotb;
        }
      }
      __syncthreads();
      for (int e = wv; e < nE; e += nw) {  // position cotangents go to both ends, movable or not
        const int r0 = sgpr((int)T[A.o_cur + c * nE + e]), r1 = sgpr((int)T[A.o_cur + (c + 1) * nE + e]);
        if (r0 == r1) continue;
        float* R = L + sgpr((int)T[A.o_ent + e * EW + 2]) * ROWF;
        const int qrow = SH ? sgpr((int)T[A.o_ent + e * EW + 4]) : -1;
        v2 pb = V(R[0], R[ROWF]);
        float rb = qrow >= 0 ? L[qrow * ROWF] : 0.f;
        for (int r = r0; r < r1; ++r) {
          const uint32_t rf = (uint32_t)sgpr((int)T[A.o_ref + r]);
          const int row = A.row_pairs + (int)((rf >> REF_ROW_SHIFT) & REF_ROW);
          if (SH && (rf & REF_SHAPED)) {  // its own rows for either end
            pb = pb + row2((rf >> 31) ? row + 2 : row);
            if (!(rf >> 31)) rb = rb + L[(row + 4) * ROWF];
          } else {
            const v2 db = row2(row);
            pb = (rf >> 31) ? pb - db : pb + db;
          }
        }
        R[0] = pb.x; R[ROWF] = pb.y;
        if (qrow >= 0) L[qrow * ROWF] = rb;
      }
      __syncthreads();
    }
  }

  // ---- out: state cotangents (rotation in closed form), then the force cotangents pulled back through the action clamps
  for (int e = wv; e < nE; e += nw) {
    const Ent D = load_ent<SH>(T + A.o_ent + e * EW);
    const float* G = g_state_out + (long)e * 6 * ld + env;
    const float* R = L + D.arow * ROWF;
    const bool mov = D.flags & VMAS_F_MOVABLE, rotb = D.flags & VMAS_F_ROTATABLE;
    const v2 vb = mov ? V(R[2 * ROWF], R[3 * ROWF]) : V(G[2 * ld], G[3 * ld]);
    float rb = G[4 * ld], ab = G[5 * ld], Tb = 0.f;
    if (SH && D.qrow >= 0) {  // swept with the substeps
      const float* Q = L + D.qrow * ROWF;
      rb = Q[0]; ab = Q[1 * ROWF]; Tb = Q[3 * ROWF];
    } else if (rotb)  // ang_vel' = ang_vel (1 - drag on substep 0) + Tq / I dt, rot' = rot + ang_vel' dt
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
        const v2 f1 = clamp_action_force(raw, D.flags & VMAS_F_MAX_F, D.max_f, D.flags & VMAS_F_F_RANGE, D.f_range).f1;
        fb = V(pass_clamp(f1.x, D.f_range, fb.x), pass_clamp(f1.y, D.f_range, fb.y));
      }
      if (D.flags & VMAS_F_MAX_F) fb = clamp_with_norm_vjp(raw, D.max_f, fb);
    }
    if (rotb) {
      tb = tb + Tb;
      const action_torque_t t = clamp_action_torque(ft_in[ao + 2 * ld + env], D.flags & VMAS_F_MAX_T, D.max_t, D.flags & VMAS_F_T_RANGE,
                                                    D.t_range);
      if (D.flags & VMAS_F_T_RANGE) tb = pass_clamp(t.t1, D.t_range, tb);
      tb = t.over ? 0.f : tb;  // t / |t| max_t does not depend on |t|
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
    if (pairs[p].type != VMAS_PAIR_SS && pairs[p].type != VMAS_PAIR_LS && pairs[p].type != VMAS_PAIR_BS)
      return refuse("pair %d (entities %d, %d) has type %d, the backward kernel serves sphere-sphere, line-sphere and box-sphere "
                    "pairs only (line-line, box-line and box-box pairs are out of its scope)", p, pairs[p].a, pairs[p].b,
                    pairs[p].type);
  if (n_joints > 0) return refuse("the world has %d joint constraint(s), which the backward kernel does not serve", n_joints);
  for (int e = 0; e < nE; ++e)
    if (ents[e].flags & (VMAS_F_LIN_FRICTION | VMAS_F_ANG_FRICTION))
      return refuse("entity %d has %s friction, which the backward kernel does not serve", e,
                    (ents[e].flags & VMAS_F_LIN_FRICTION) ? "linear" : "angular");
  // pairs that exert no force or torque on anything that moves or turns get no cotangent: left out
  std::vector<int> kept;
  std::vector<char> shaped(nE, 0);  // a line or box that is `a` of a kept line-sphere / box-sphere pair
  for (int p = 0; p < nP_all; ++p) {
    const bool sh = pairs[p].type != VMAS_PAIR_SS;
    if (((ents[pairs[p].a].flags | ents[pairs[p].b].flags) & VMAS_F_MOVABLE) || (sh && (ents[pairs[p].a].flags & VMAS_F_ROTATABLE))) {
      kept.push_back(p);
      if (sh) { shaped[pairs[p].a] = 1; P.shapes = true; }
    }
  }
  P.nP = (int)kept.size();
  if (P.nP > (int)REF_IDX) return refuse("the world has %d pairs, the backward kernel's tables index %d", P.nP, (int)REF_IDX);
  // tile rows
  std::vector<int> arow(nE), prow(nE), qrow(nE, -1);
  int rows = 0, n_own = 0;
  for (int e = 0; e < nE; ++e) {
    const bool mov = ents[e].flags & VMAS_F_MOVABLE, rot = ents[e].flags & VMAS_F_ROTATABLE;
    arow[e] = rows;
    prow[e] = rows + (mov ? 8 : 2);
    rows += mov ? 8 + 4 * C.substeps : 4;
    if (shaped[e]) {  // rot / ang_vel / torque cotangents, cos/sin rows, rot per substep where it changes
      qrow[e] = rows;
      rows += 4 + (ents[e].shape == VMAS_SHAPE_BOX ? 4 : 2) + (rot ? C.substeps : 1);
    }
    n_own += mov || (shaped[e] && rot);
  }
  std::vector<int> prows(P.nP);
  int all_rows = 0;
  for (int i = 0; i < P.nP; ++i) all_rows += prows[i] = pairs[kept[i]].type == VMAS_PAIR_SS ? SS_ROWS : SHAPE_ROWS;
  const size_t row_bytes = ROWF * sizeof(float), ent_bytes = (size_t)rows * row_bytes;
  const int want = P.nP < MAX_WAVES ? P.nP : MAX_WAVES;  // a run of fewer pairs than waves would idle most of the block
  size_t want_bytes = 0;                                  // (the first run starts with the first pairs)
  for (int i = 0; i < want; ++i) want_bytes += prows[i] * row_bytes;
  if (P.shapes && want_bytes < SHAPE_ROWS * row_bytes) want_bytes = SHAPE_ROWS * row_bytes;  // (every later pair must fit a run too)
  if (ent_bytes + want_bytes > kLdsMax)
    return refuse("a 64-environment tile needs %zu B of LDS for the adjoint and checkpoint rows of %d entities over %d substeps "
                  "and %zu B for the rows of %d pairs, the compute unit has %zu B", ent_bytes, nE, C.substeps,
                  want_bytes, want, kLdsMax);
  // runs of pairs: as few as the rows left allow, then as even as they can be (the smallest run size that still gives that
  // many runs); pairs stay in pair order
  const int room = (int)((kLdsMax - ent_bytes) / row_bytes);
  std::vector<int> starts;
  auto cut = [&](int cap) {
    starts.assign(1, 0);
    for (int i = 0, used = 0; i < P.nP; ++i) {
      if (used + prows[i] > cap) { starts.push_back(i); used = 0; }
      used += prows[i];
    }
    starts.push_back(P.nP);
    return (int)starts.size() - 1;
  };
  P.n_chunks = cut(room);
  for (int cap = (all_rows + P.n_chunks - 1) / P.n_chunks; cap < room && cut(cap) > P.n_chunks; ++cap) {}
  if ((int)starts.size() - 1 > P.n_chunks) cut(room);
  std::vector<int> roff(P.nP);
  int chunk_rows = 0;
  P.chunk = 0;
  for (int c = 0; c < P.n_chunks; ++c) {
    int used = 0;
    for (int i = starts[c]; i < starts[c + 1]; ++i) { roff[i] = used; used += prows[i]; }
    chunk_rows = used > chunk_rows ? used : chunk_rows;
    P.chunk = starts[c + 1] - starts[c] > P.chunk ? starts[c + 1] - starts[c] : P.chunk;
  }
  P.row_pairs = rows;
  P.n_rows = rows + chunk_rows;
  P.lds_bytes = (size_t)P.n_rows * row_bytes;
  const int work = n_own > P.chunk ? n_own : P.chunk;
  P.nw = work < 1 ? 1 : (work > MAX_WAVES ? MAX_WAVES : work);
  // the table
  std::vector<uint32_t>& T = P.table;
  P.o_ent = 0;
  T.assign((size_t)nE * EW, 0u);
  for (int e = 0; e < nE; ++e) {
    const VmasEntityDesc& s = ents[e];
    uint32_t* w = &T[(size_t)e * EW];
    w[0] = s.flags; w[1] = (uint32_t)s.agent_index; w[2] = (uint32_t)arow[e]; w[3] = (uint32_t)prow[e]; w[4] = (uint32_t)qrow[e];
    w[5] = fbits(s.mass); w[6] = fbits(s.inertia); w[7] = fbits(s.one_minus_drag);
    w[8] = fbits(s.max_speed); w[9] = fbits(s.v_range); w[10] = fbits(s.gravity[0]); w[11] = fbits(s.gravity[1]);
    w[12] = fbits(s.max_f); w[13] = fbits(s.f_range); w[14] = fbits(s.max_t); w[15] = fbits(s.t_range);
    w[16] = shaped[e] ? (s.shape == VMAS_SHAPE_BOX ? 4u : 2u) : 0u;
  }
  P.o_pair = (int)T.size();
  for (int i = 0; i < P.nP; ++i) {
    const VmasPairDesc& pr = pairs[kept[i]];
    const int a = pr.a, b = pr.b;
    const VmasEntityDesc &ea = ents[a], &eb = ents[b];
    const bool ma = ea.flags & VMAS_F_MOVABLE, mb = eb.flags & VMAS_F_MOVABLE;
    uint32_t w[PW] = {(uint32_t)prow[a], ma ? 4u : 0u, (uint32_t)prow[b], mb ? 4u : 0u,
                      fbits(ea.radius + eb.radius),  // (fp32 sum, as the forward's items carry it)
                      (uint32_t)(ma ? arow[a] + 4 : -1), (uint32_t)(mb ? arow[b] + 4 : -1), (uint32_t)pr.type, (uint32_t)roff[i]};
    if (pr.type != VMAS_PAIR_SS) {  // the forward's item of the pair (build_items, vmas_hip.hip): b's radius + LINE_MIN_DIST, a's dimensions
      w[4] = fbits(eb.radius + kLineMinDist);
      if (pr.type == VMAS_PAIR_BS && (ea.flags & VMAS_F_HOLLOW)) w[7] |= PT_HOLLOW;
      w[9] = (uint32_t)(qrow[a] + 4);
      w[10] = (uint32_t)((ea.flags & VMAS_F_ROTATABLE) ? qrow[a] + 2 : -1);
      w[11] = fbits(pr.type == VMAS_PAIR_LS ? ea.length / 2.f : ea.length);
      w[12] = fbits(ea.width);
    }
    T.insert(T.end(), w, w + PW);
  }
  // per entity its pairs in pair order (REF_*), and where each chunk's run of them starts
  P.o_ref = (int)T.size();
  std::vector<int> ref_begin(nE + 1, 0);
  for (int e = 0; e < nE; ++e) {
    ref_begin[e] = (int)T.size() - P.o_ref;
    for (int i = 0; i < P.nP; ++i) {
      const uint32_t rf = (uint32_t)i | (uint32_t)roff[i] << REF_ROW_SHIFT | (prows[i] == SHAPE_ROWS ? REF_SHAPED : 0u);
      if (pairs[kept[i]].a == e) T.push_back(rf);
      else if (pairs[kept[i]].b == e) T.push_back(rf | 0x80000000u);
    }
  }
  ref_begin[nE] = (int)T.size() - P.o_ref;
  P.o_cur = (int)T.size();
  for (int c = 0; c <= P.n_chunks; ++c)
    for (int e = 0; e < nE; ++e) {
      int r = ref_begin[e];
      while (r < ref_begin[e + 1] && (int)(T[P.o_ref + r] & REF_IDX) < starts[c]) ++r;
      T.push_back((uint32_t)(c == P.n_chunks ? ref_begin[e + 1] : r));
    }
  P.o_chk = (int)T.size();
  for (int c = 0; c <= P.n_chunks; ++c) T.push_back((uint32_t)starts[c]);
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
      if (hipFuncSetAttribute((const void*)step_vjp_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess ||
          hipFuncSetAttribute((const void*)step_vjp_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess)
        return host_fail("vmas_world_step_vjp: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      set_for = kLdsMax;
    }
  }
  Args A;
  A.C = p.C;
  A.nE = p.nE; A.n_chunks = p.n_chunks; A.row_pairs = p.row_pairs;
  A.o_ent = p.o_ent; A.o_pair = p.o_pair; A.o_ref = p.o_ref; A.o_cur = p.o_cur; A.o_chk = p.o_chk;
  A.tab = p.d_table;
  const dim3 grid((batch + ROWF - 1) / ROWF), block(ROWF * p.nw);
  if (p.shapes)
    hipLaunchKernelGGL(step_vjp_kernel<true>, grid, block, p.lds_bytes, s, A, state_in, ft_in, ld, g_state_out, g_ft_out, g_state_in,
                       g_ft_in, batch);
  else
    hipLaunchKernelGGL(step_vjp_kernel<false>, grid, block, p.lds_bytes, s, A, state_in, ft_in, ld, g_state_out, g_ft_out, g_state_in,
                       g_ft_in, batch);
  if (hipGetLastError() != hipSuccess) return host_fail("vmas_world_step_vjp: launch of the backward kernel failed");
  return 0;
}

}  // namespace vjp
}  // namespace vmas
