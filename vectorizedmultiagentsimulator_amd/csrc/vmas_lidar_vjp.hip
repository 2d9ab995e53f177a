// vmas_lidar_vjp.hip - the backward kernel of World.cast_rays: one launch computes the vector-Jacobian product of one
// vmas_world_cast_rays for the registered sensor set (include/vmas_hip.h, vmas_world_cast_rays_vjp).
//
// Lane = environment, a block owns a tile of 64 environments.  The position and rotation rows of every entity that casts
// or is seen ("slot") are staged into LDS once.  Work units are (sensor, ray chunk), dealt round-robin over the tile's
// waves.  A unit walks its rays in ascending order, four at a time: it recomputes every target's distance with the
// forward's own expressions (lidar_cast_chunk, vmas_env_device.h - restated here, the forward is not touched), keeps the
// running minimum and ITS target per lane, and then evaluates the adjoint of that one target only - torch.min(dim)'s rule;
// a ray whose minimum stayed at max_range sends its cotangent nowhere.  The winner differs per lane: the wave loops over
// the distinct winners present (readlane of the first pending lane), so target records are wave-uniform loads and the
// shape branch is uniform.
//
// A unit adds into accumulator rows of its own: 3 for the carrier (x, y, rotation), 2 per sphere target, 3 per line or box
// target.  After a block barrier the owner of each slot adds the rows that refer to it - in sensor registration order, then
// chunk order, within a unit the carrier's before the targets' - onto its carried sum.  No atomics: two runs on the same
// inputs are bitwise equal.  When the rows of all units do not fit in the compute unit's LDS the sensors are processed in
// runs of as many as fit; the carried sums make the order of the additions - and so the bits - independent of the split.
// Tiles never talk to each other: block barriers only.
//
// Tile rows (64 floats each):  slot s: 3 s .. 3 s + 2  x, y, rotation  |  3 n_slots + the same: the carried sums  |  the rows of
// a run's units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "vmas_device.h"
#include "vmas_lidar_vjp.h"

namespace vmas {
int host_fail(const char* msg);  // vmas_hip.hip: sets vmas_last_error(), returns -1

namespace lidar_vjp {
namespace {

constexpr int ROWF = 64;                 // floats per LDS row = environments per tile
constexpr int RC = 4;                    // rays a unit holds in registers at a time
constexpr int SW = 10, TW = 6, UW = 4;   // table words per sensor / target / unit
constexpr int CARRIER_ROWS = 3, SPHERE_ROWS = 2, SHAPE_ROWS = 3;
constexpr uint32_t REF_ROT = 1u << 31;   // an owner's reference: first row | REF_ROT (the third row is a rotation's)
constexpr int MAX_WAVES = 8;
constexpr size_t kLdsMax = 160 * 1024;   // LDS of one gfx950 CU
constexpr int kSphereShape = 0, kBoxShape = 1;  // == VMAS_SHAPE_* of include/vmas_hip.h (anything else: a line)

struct Args {
  int32_t n_slots, n_runs, max_rays;
  int32_t o_slot, o_sens, o_unit, o_run, o_cur, o_ref;
  const uint32_t* tab;
};

VD int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
VD int word(const uint32_t* p) { return sgpr((int)*p); }
VD float fword(const uint32_t* p) { return __uint_as_float((uint32_t)sgpr((int)*p)); }

// ---- the forward's distances, expression for expression lidar_cast_chunk's, with what their adjoints need
struct SphereHit { float dist, t, m; v2 u; bool ok; };
VD SphereHit sphere_ray(v2 o, v2 tpos, float radius, float half_range, float c, float s) {  // core.py:1414-1490
  SphereHit h;
  h.u = tpos - o;
  const v2 dir = V(c, s);
  const v2 lp = V(o.x + dir.x * half_range, o.y + dir.y * half_range);
  const v2 cp = closest_point_line<false>(lp, c, s, 0.f, tpos);
  const float dn = vnorm(tpos - cp);
  h.ok = (dn < radius) && (vdot(h.u, dir) > 0.f);
  const float a = radius * radius - dn * dn;
  h.m = sqrt_n(a > 0.f ? a : 1e-8f);
  h.t = vnorm(cp - o);
  h.dist = h.t - h.m;
  return h;
}

struct BoxFrame { float cn, sn, cp, sp; v2 p; };
VD BoxFrame box_frame(v2 o, v2 tpos, float trot) {
  BoxFrame f;
  f.cn = cosf(-trot); f.sn = sinf(-trot); f.cp = cosf(trot); f.sp = sinf(trot);
  f.p = rotate(o - tpos, f.cn, f.sn);
  return f;
}
struct BoxHit { float dist, t0; v2 q, ia; bool ok, xslab; };
VD BoxHit box_ray(const BoxFrame& f, v2 o, v2 tpos, float length, float width, float c, float s) {  // core.py:1281-1372
  BoxHit h;
  h.q = rotate(V(c, s), f.cn, f.sn);
  const float tx1 = (-length / 2.f - f.p.x) / h.q.x, tx2 = (length / 2.f - f.p.x) / h.q.x;
  const float ty1 = (-width / 2.f - f.p.y) / h.q.y, ty2 = (width / 2.f - f.p.y) / h.q.y;
  const float ax = min_t(tx1, tx2), ay = min_t(ty1, ty2);
  h.t0 = max_t(ax, ay);
  h.xslab = ax > ay;  // (the operand max_t returns)
  const float t1 = min_t(max_t(tx1, tx2), max_t(ty1, ty2));
  h.ia = V(h.t0 * h.q.x + f.p.x, h.t0 * h.q.y + f.p.y);
  const v2 iw = rotate(h.ia, f.cp, f.sp) + tpos;
  h.dist = vnorm(o - iw);
  h.ok = (t1 >= h.t0) && (h.t0 > 0.f);
  return h;
}

struct LineHit { float dist, rxs, uu; bool ok; };
VD LineHit line_ray(v2 rr, v2 qo, float c, float s) {  // core.py:1544-1626
  LineHit h;
  const v2 dir = V(c, s);
  h.rxs = vcross(rr, dir);
  const float tt = vcross(qo, V(dir.x / h.rxs, dir.y / h.rxs));
  h.uu = vcross(qo, V(rr.x / h.rxs, rr.y / h.rxs));
  h.dist = norm2(h.uu * dir.x, h.uu * dir.y);
  h.ok = !(h.rxs == 0.f || tt > 0.5f || tt < -0.5f || h.uu < 0.f);
  return h;
}

// One unit: rays [r0, r1) of sensor l, into the unit's own rows.
VD void cast_unit(const Args& A, const uint32_t* __restrict__ T, float* L, const float2* __restrict__ angles_cs,
                  const float* __restrict__ g_out, long ld, int env, bool live, int lane, int u) {
  const uint32_t* U = T + A.o_unit + u * UW;
  const int l = word(U), r0 = word(U + 1), r1 = word(U + 2);
  float* acc = L + word(U + 3) * ROWF + lane;
  const uint32_t* S = T + A.o_sens + l * SW;
  const int cslot = word(S), n_rays = word(S + 1), n_t = word(S + 2), t_off = word(S + 3), a_off = word(S + 4),
            cs_off = word(S + 5), urows = word(S + 8);
  const float R = fword(S + 6), half_range = fword(S + 7);
  for (int i = 0; i < urows; ++i) acc[i * ROWF] = 0.f;
  const float* P = L + lane;  // the staged rows
  const v2 o = V(P[cslot * 3 * ROWF], P[(cslot * 3 + 1) * ROWF]);
  const float arot = P[(cslot * 3 + 2) * ROWF];
  const bool table = __all(arot == 0.f);  // (see lidar_cast_chunk: the same sincosf made the table)
  v2 ob = V(0.f, 0.f);  // the carrier's cotangents, summed over the unit's rays in ray order
  float rb = 0.f;

  for (int rc = r0; rc < r1; rc += RC) {
    float c[RC], s[RC], best[RC];
    int win[RC];
#pragma unroll
    for (int i = 0; i < RC; ++i) {
      const int r = rc + i < n_rays ? rc + i : n_rays - 1;
      if (table) {
        const float2 cs = angles_cs[cs_off + r];
        c[i] = cs.x; s[i] = cs.y;
      } else {
        const float th = fword(T + a_off + r) + arot;  // sensors.py:118
        sincosf(th, &s[i], &c[i]);
      }
      best[i] = R;  // core.py:1672-1674
      win[i] = -1;
    }
    // ---- the forward again: the minimum and its target (the first in target order at a tie)
    for (int ti = 0; ti < n_t; ++ti) {
      const uint32_t* G = T + t_off + ti * TW;
      const int slot = word(G), shape = word(G + 1);
      const v2 tpos = V(P[slot * 3 * ROWF], P[(slot * 3 + 1) * ROWF]);
      if (shape == kSphereShape) {
        const float radius = fword(G + 4);
        const float dx = tpos.x - o.x, dy = tpos.y - o.y, lim = R + radius + 1e-4f;
        const bool near = !(dx * dx + dy * dy > lim * lim);  // a sphere out of reach cannot lower the minimum: skipped, as the forward does
        if (!__any(near)) continue;
#pragma unroll
        for (int i = 0; i < RC; ++i) {
          const SphereHit h = sphere_ray(o, tpos, radius, half_range, c[i], s[i]);
          if (near && h.ok && h.dist < best[i]) { best[i] = h.dist; win[i] = ti; }
        }
      } else if (shape == kBoxShape) {
        const BoxFrame f = box_frame(o, tpos, P[(slot * 3 + 2) * ROWF]);
        const float length = fword(G + 2), width = fword(G + 3);
#pragma unroll
        for (int i = 0; i < RC; ++i) {
          const BoxHit h = box_ray(f, o, tpos, length, width, c[i], s[i]);
          if (h.ok && h.dist < best[i]) { best[i] = h.dist; win[i] = ti; }
        }
      } else {
        const float trot = P[(slot * 3 + 2) * ROWF], length = fword(G + 2);
        const v2 rr = V(cosf(trot) * length, sinf(trot) * length), qo = o - tpos;
#pragma unroll
        for (int i = 0; i < RC; ++i) {
          const LineHit h = line_ray(rr, qo, c[i], s[i]);
          if (h.ok && h.dist < best[i]) { best[i] = h.dist; win[i] = ti; }
        }
      }
    }
    // ---- the adjoint of each ray's winner
#pragma unroll
    for (int i = 0; i < RC; ++i) {
      const int r = rc + i;
      if (r >= n_rays) break;  // (padding rows of g_out contribute nothing)
      const float g = live ? g_out[((long)l * A.max_rays + r) * ld + env] : 0.f;
      int w = win[i];
      const v2 dir = V(c[i], s[i]);
      unsigned long long pending;
      while ((pending = __ballot(w >= 0)) != 0ull) {
        const int ti = __builtin_amdgcn_readlane(w, __ffsll((long long)pending) - 1);
        const bool me = w == ti;
        w = me ? -1 : w;
        const uint32_t* G = T + t_off + ti * TW;
        const int slot = word(G), shape = word(G + 1);
        float* tacc = acc + word(G + 5) * ROWF;
        const v2 tpos = V(P[slot * 3 * ROWF], P[(slot * 3 + 1) * ROWF]);
        v2 obar, dirbar;   // cotangents of the ray's origin and direction
        float trotbar = 0.f;
        if (shape == kSphereShape) {
          // dist = t - sqrt(r^2 - |u|^2 + t^2), u = tpos - o, t = u . dir
          const SphereHit h = sphere_ray(o, tpos, fword(G + 4), half_range, c[i], s[i]);
          const float k = g * (1.f - h.t / h.m), gm = g / h.m;
          obar = V(0.f - (k * dir.x + gm * h.u.x), 0.f - (k * dir.y + gm * h.u.y));
          dirbar = V(k * h.u.x, k * h.u.y);
        } else if (shape == kBoxShape) {
          // dist = t0 = (+-size / 2 - p) / q of the slab that wins, p = R(-rot) (o - tpos), q = R(-rot) dir
          const BoxFrame f = box_frame(o, tpos, P[(slot * 3 + 2) * ROWF]);
          const BoxHit h = box_ray(f, o, tpos, fword(G + 2), fword(G + 3), c[i], s[i]);
          const float qk = h.xslab ? h.q.x : h.q.y;
          const float pk = (0.f - g) / qk, qb = (0.f - g) * h.t0 / qk;
          const v2 pbar = h.xslab ? V(pk, 0.f) : V(0.f, pk), qbar = h.xslab ? V(qb, 0.f) : V(0.f, qb);
          obar = rotate(pbar, f.cp, f.sp);
          dirbar = rotate(qbar, f.cp, f.sp);
          trotbar = (pbar.x * f.p.y - pbar.y * f.p.x) + (qbar.x * h.q.y - qbar.y * h.q.x);
        } else {
          // dist = uu = (qo x rr) / (rr x dir), qo = o - tpos, rr = length (cos rot, sin rot)
          const float trot = P[(slot * 3 + 2) * ROWF], length = fword(G + 2);
          const v2 rr = V(cosf(trot) * length, sinf(trot) * length), qo = o - tpos;
          const LineHit h = line_ray(rr, qo, c[i], s[i]);
          const float nb = g / h.rxs, xb = (0.f - g) * h.uu / h.rxs;
          obar = V(nb * rr.y, 0.f - nb * rr.x);
          dirbar = V(0.f - xb * rr.y, xb * rr.x);
          const v2 rrbar = V(xb * dir.y - nb * qo.y, nb * qo.x - xb * dir.x);
          trotbar = rrbar.y * rr.x - rrbar.x * rr.y;
        }
        const float thbar = dirbar.y * dir.x - dirbar.x * dir.y;  // th = angle + rotation of the carrier
        ob = V(ob.x + (me ? obar.x : 0.f), ob.y + (me ? obar.y : 0.f));
        rb = rb + (me ? thbar : 0.f);
        tacc[0] = tacc[0] - (me ? obar.x : 0.f);  // (every target's position enters through tpos - o or o - tpos)
        tacc[ROWF] = tacc[ROWF] - (me ? obar.y : 0.f);
        if (shape != kSphereShape) tacc[2 * ROWF] = tacc[2 * ROWF] + (me ? trotbar : 0.f);
      }
    }
  }
  acc[0] = ob.x; acc[ROWF] = ob.y; acc[2 * ROWF] = rb;
}

__global__ __launch_bounds__(ROWF* MAX_WAVES) void cast_rays_vjp_kernel(Args A, const float2* __restrict__ angles_cs,
                                                                        const float* __restrict__ state, long ld,
                                                                        const float* __restrict__ g_out,
                                                                        float* __restrict__ g_state, int batch) {
  extern __shared__ float L[];
  const uint32_t* __restrict__ T = A.tab;
  const int lane = threadIdx.x & (ROWF - 1), wv = sgpr((int)(threadIdx.x / ROWF)), nw = (int)(blockDim.x / ROWF);
  const int env0 = (int)blockIdx.x * ROWF + lane;
  const bool live = env0 < batch;
  const int env = live ? env0 : batch - 1;
  const int ns = A.n_slots;
  for (int i = wv; i < ns * 3; i += nw) {
    const int e = word(T + A.o_slot + i / 3), f = i % 3;
    L[i * ROWF + lane] = state[((long)e * 6 + (f == 2 ? 4 : f)) * ld + env];
    L[(ns * 3 + i) * ROWF + lane] = 0.f;
  }
  __syncthreads();
  for (int run = 0; run < A.n_runs; ++run) {
    const int u1 = word(T + A.o_run + run + 1);
    for (int u = word(T + A.o_run + run) + wv; u < u1; u += nw) cast_unit(A, T, L, angles_cs, g_out, ld, env, live, lane, u);
    __syncthreads();
    for (int sl = wv; sl < ns; sl += nw) {  // the owner of slot sl
      float* own = L + (ns + sl) * 3 * ROWF + lane;
      float x = own[0], y = own[ROWF], rot = own[2 * ROWF];
      const int k1 = word(T + A.o_cur + run * ns + sl + 1);
      for (int k = word(T + A.o_cur + run * ns + sl); k < k1; ++k) {
        const uint32_t rf = (uint32_t)word(T + A.o_ref + k);
        const float* row = L + (int)(rf & ~REF_ROT) * ROWF + lane;
        x = x + row[0]; y = y + row[ROWF];
        if (rf & REF_ROT) rot = rot + row[2 * ROWF];
      }
      if (run + 1 < A.n_runs) {
        own[0] = x; own[ROWF] = y; own[2 * ROWF] = rot;
      } else if (live) {
        float* O = g_state + (long)word(T + A.o_slot + sl) * 6 * ld + env0;
        O[0] = x; O[ld] = y; O[4 * ld] = rot;
      }
    }
    if (run + 1 < A.n_runs) __syncthreads();
  }
}

uint32_t fbits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

}  // namespace

void make_plan(const Sensor* sensors, int n, const Target* targets, const float* angles, int n_entities, Plan* out) {
  Plan& P = *out;
  P = Plan{};
  auto refuse = [&](const char* fmt, auto... a) { snprintf(P.why, sizeof(P.why), fmt, a...); };
  if (n <= 0) return refuse("%s", "no sensors registered (vmas_world_set_lidars)");
  P.n_lidars = n;
  // slots: every entity that casts or is seen, in order of first appearance
  std::vector<int> ent_slot(n_entities, -1), slot_ent;
  auto slot = [&](int e) { if (ent_slot[e] < 0) { ent_slot[e] = (int)slot_ent.size(); slot_ent.push_back(e); } return ent_slot[e]; };
  std::vector<int> urows(n, CARRIER_ROWS);  // accumulator rows of one unit of sensor l
  int n_angles = 0, n_targets = 0;
  for (int l = 0; l < n; ++l) {
    slot(sensors[l].entity);
    for (int t = 0; t < sensors[l].n_targets; ++t) {
      const Target& G = targets[sensors[l].target_off + t];
      slot(G.entity);
      urows[l] += G.shape == kSphereShape ? SPHERE_ROWS : SHAPE_ROWS;
    }
    P.max_rays = sensors[l].n_rays > P.max_rays ? sensors[l].n_rays : P.max_rays;
    n_angles += sensors[l].n_rays;
    n_targets += sensors[l].n_targets;
  }
  P.n_slots = (int)slot_ent.size();
  const size_t row_bytes = ROWF * sizeof(float), fixed_bytes = (size_t)P.n_slots * 6 * row_bytes;
  const int room = fixed_bytes < kLdsMax ? (int)((kLdsMax - fixed_bytes) / row_bytes) : 0;
  // rays per unit: few sensors are split into ray chunks so that a tile has a unit for each of its waves; a sensor whose
  // chunks' rows do not fit one run together is the reason to try whole sensors
  auto round4 = [](int x) { return (x + RC - 1) / RC * RC; };
  const int split = n >= MAX_WAVES ? 1 : (MAX_WAVES + n - 1) / n;
  P.unit_rays = round4((P.max_rays + split - 1) / split);
  auto units_of = [&](int l) { return (sensors[l].n_rays + P.unit_rays - 1) / P.unit_rays; };
  auto fits = [&]() { for (int l = 0; l < n; ++l) if (units_of(l) * urows[l] > room) return l; return -1; };
  if (fits() >= 0) P.unit_rays = round4(P.max_rays);
  if (const int l = fits(); l >= 0)
    return refuse("a 64-environment tile needs %zu B of LDS for the staged and carried rows of %d entities and %zu B for the "
                  "accumulator rows of sensor %d (%d targets), the compute unit has %zu B", fixed_bytes, P.n_slots,
                  (size_t)urows[l] * row_bytes, l, sensors[l].n_targets, kLdsMax);
  // runs of sensors, in registration order: as few as the rows left allow
  std::vector<int> run_unit(1, 0), unit_sensor, unit_row;
  int used = 0, run_rows = 0, run_units = 0;
  for (int l = 0; l < n; ++l) {
    const int k = units_of(l);
    if (used + k * urows[l] > room) { run_unit.push_back((int)unit_sensor.size()); used = 0; }
    for (int j = 0; j < k; ++j) { unit_sensor.push_back(l); unit_row.push_back(P.n_slots * 6 + used + j * urows[l]); }
    used += k * urows[l];
    run_rows = used > run_rows ? used : run_rows;
    const int in_run = (int)unit_sensor.size() - run_unit.back();
    run_units = in_run > run_units ? in_run : run_units;
  }
  run_unit.push_back((int)unit_sensor.size());
  P.n_units = (int)unit_sensor.size();
  P.n_runs = (int)run_unit.size() - 1;
  P.n_rows = P.n_slots * 6 + run_rows;
  P.lds_bytes = (size_t)P.n_rows * row_bytes;
  const int work = run_units > P.n_slots ? run_units : P.n_slots;
  P.nw = work > MAX_WAVES ? MAX_WAVES : work;
  // the table
  std::vector<uint32_t>& T = P.table;
  P.o_slot = 0;
  for (int e : slot_ent) T.push_back((uint32_t)e);
  P.o_sens = (int)T.size();
  const int o_targets = P.o_sens + n * SW, o_angles = o_targets + n_targets * TW;
  T.resize((size_t)o_angles + n_angles, 0u);
  for (int i = 0; i < n_angles; ++i) T[o_angles + i] = fbits(angles[i]);
  for (int l = 0; l < n; ++l) {
    const Sensor& S = sensors[l];
    uint32_t* w = &T[P.o_sens + (size_t)l * SW];
    w[0] = (uint32_t)ent_slot[S.entity]; w[1] = (uint32_t)S.n_rays; w[2] = (uint32_t)S.n_targets;
    w[3] = (uint32_t)(o_targets + S.target_off * TW); w[4] = (uint32_t)(o_angles + S.angle_off); w[5] = (uint32_t)S.angle_off;
    w[6] = fbits(S.max_range); w[7] = fbits(S.half_range); w[8] = (uint32_t)urows[l];
    int row = CARRIER_ROWS;
    for (int t = 0; t < S.n_targets; ++t) {
      const Target& G = targets[S.target_off + t];
      uint32_t* g = &T[o_targets + (size_t)(S.target_off + t) * TW];
      g[0] = (uint32_t)ent_slot[G.entity]; g[1] = (uint32_t)G.shape; g[2] = fbits(G.length); g[3] = fbits(G.width);
      g[4] = fbits(G.radius); g[5] = (uint32_t)row;
      row += G.shape == kSphereShape ? SPHERE_ROWS : SHAPE_ROWS;
    }
  }
  P.o_unit = (int)T.size();
  for (int u = 0, j = 0; u < P.n_units; ++u) {
    const int l = unit_sensor[u];
    j = (u > 0 && unit_sensor[u - 1] == l) ? j + 1 : 0;
    const int r0 = j * P.unit_rays, r1 = r0 + P.unit_rays < sensors[l].n_rays ? r0 + P.unit_rays : sensors[l].n_rays;
    const uint32_t w[UW] = {(uint32_t)l, (uint32_t)r0, (uint32_t)r1, (uint32_t)unit_row[u]};
    T.insert(T.end(), w, w + UW);
  }
  P.o_run = (int)T.size();
  for (int r : run_unit) T.push_back((uint32_t)r);
  // per (run, slot) the rows that refer to the slot: units in order, within a unit the carrier's rows, then the targets'
  std::vector<uint32_t> cur, ref;
  for (int run = 0; run < P.n_runs; ++run)
    for (int sl = 0; sl < P.n_slots; ++sl) {
      cur.push_back((uint32_t)ref.size());
      for (int u = run_unit[run]; u < run_unit[run + 1]; ++u) {
        const Sensor& S = sensors[unit_sensor[u]];
        if (ent_slot[S.entity] == sl) ref.push_back((uint32_t)unit_row[u] | REF_ROT);
        for (int t = 0; t < S.n_targets; ++t) {
          const Target& G = targets[S.target_off + t];
          if (ent_slot[G.entity] == sl)
            ref.push_back((uint32_t)(unit_row[u] + (int)T[o_targets + (size_t)(S.target_off + t) * TW + 5]) |
                          (G.shape == kSphereShape ? 0u : REF_ROT));
        }
      }
    }
  cur.push_back((uint32_t)ref.size());
  P.o_cur = (int)T.size();
  T.insert(T.end(), cur.begin(), cur.end());
  P.o_ref = (int)T.size();
  T.insert(T.end(), ref.begin(), ref.end());
  P.ok = true;
}

int upload(Plan* p) {
  if (hipMalloc((void**)&p->d_table, p->table.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(p->d_table, p->table.data(), p->table.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    return host_fail("vmas_world_set_lidars: uploading the LIDAR backward kernel's table failed");
  return 0;
}

void release(Plan* p) {
  if (p->d_table) (void)hipFree(p->d_table);
  p->d_table = nullptr;
}

int launch(const Plan& p, int device, int batch, const float2* angles_cs, const float* state, long ld, const float* g_out,
           float* g_state, hipStream_t s) {
  if (!p.ok || !p.d_table) return host_fail("vmas_world_cast_rays_vjp: the sensor set has no backward plan");
  if (p.lds_bytes > 64 * 1024) {  // opt in to the large LDS once per device
    static std::atomic<size_t> set_for_dev[64];
    std::atomic<size_t>& set_for = set_for_dev[device & 63];
    if (set_for.load() < p.lds_bytes) {
      if (hipFuncSetAttribute((const void*)cast_rays_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess)
        return host_fail("vmas_world_cast_rays_vjp: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      set_for = kLdsMax;
    }
  }
  Args A;
  A.n_slots = p.n_slots; A.n_runs = p.n_runs; A.max_rays = p.max_rays;
  A.o_slot = p.o_slot; A.o_sens = p.o_sens; A.o_unit = p.o_unit; A.o_run = p.o_run; A.o_cur = p.o_cur; A.o_ref = p.o_ref;
  A.tab = p.d_table;
  hipLaunchKernelGGL(cast_rays_vjp_kernel, dim3((batch + ROWF - 1) / ROWF), dim3(ROWF * p.nw), p.lds_bytes, s, A, angles_cs, state,
                     ld, g_out, g_state, batch);
  if (hipGetLastError() != hipSuccess) return host_fail("vmas_world_cast_rays_vjp: launch of the backward kernel failed");
  return 0;
}

}  // namespace lidar_vjp
}  // namespace vmas
