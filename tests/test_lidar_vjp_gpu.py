"""The backward kernel of World.cast_rays (csrc/vmas_lidar_vjp.hip) against torch autograd of a plain float64 restatement of
the cast on the CPU.  The bound is the rule of test_step_vjp_gpu.py: 4 x the error the SAME restatement makes in float32,
computed at run time (figures seen on one MI355X: DESIGN.md 3.3b)."""
import functools
import math

import numpy as np
import pytest
import torch
from test_step_vjp_gpu import bound_and_check, grads, packed
from test_step_vjp_gpu import restate as restate_step

from vectorizedmultiagentsimulator_amd import _abi as A
from vectorizedmultiagentsimulator_amd.core import Agent, Box, Landmark, Line, Sphere, World
from vectorizedmultiagentsimulator_amd.sensors import Lidar

pytestmark = pytest.mark.gpu
F64 = torch.float64
K = 16  # candidate environments drawn per environment: the first that meets the conditions on the inputs is taken
#: world -> seed per batch size (chosen on the CPU so that every environment finds a candidate and the coverage holds)
WORLDS = {"p": {1: 0, 64: 0, 65: 0}, "q": {63: 1, 130: 2}, "r": {65: 0}}
CASES = [(n, b) for n, seeds in WORLDS.items() for b in seeds]
f32 = lambda x: float(np.float32(x))  # noqa: E731
norm = lambda t: torch.linalg.vector_norm(t, dim=0)  # noqa: E731
cross = lambda a, b: a[0] * b[1] - a[1] * b[0]  # noqa: E731
unit = lambda th: torch.stack([torch.cos(th), torch.sin(th)])  # noqa: E731


def build_world(name, batch, device="cpu", **kw):
    """(p) a non-rotatable carrier, 5 rays over a partial fan, one ball, one bystander; (q) a box, a line and 3 rotatable agents
    with 12 rays each, one of them with a second 7-ray sensor on the landmarks only; (r) 17 agents in a ring, 3 rays each."""
    w = World(batch, device, **kw)
    if name == "p":
        w.add_landmark(Landmark("ball", shape=Sphere(0.1)))
        w.add_landmark(Landmark("mark", collide=False))
        w.add_agent(Agent("a0", rotatable=False, shape=Sphere(0.05), sensors=[
            Lidar(w, angle_start=-0.6, angle_end=0.9, n_rays=5, max_range=0.5, entity_filter=lambda e: e.name == "ball")]))
    elif name == "q":
        w.add_landmark(Landmark("box", shape=Box(0.36, 0.24)))
        w.add_landmark(Landmark("line", shape=Line(0.5)))
        for i in range(3):
            sensors = [Lidar(w, n_rays=12, max_range=0.7)]
            if i == 1:
                sensors.append(Lidar(w, angle_start=0.3, angle_end=5.0, n_rays=7, max_range=0.9,
                                     entity_filter=lambda e: isinstance(e, Landmark)))
            w.add_agent(Agent(f"a{i}", shape=Sphere(0.12), sensors=sensors))
    else:
        for i in range(17):
            w.add_agent(Agent(f"a{i}", shape=Sphere(0.04), sensors=[Lidar(w, angle_start=-0.5, angle_end=0.5, n_rays=3, max_range=0.45)]))
    return w


def make_inputs(name, n, seed):
    """Seeded candidate states [E, 6, n] in float64; environment = column // K."""
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1  # noqa: E731
    if name == "p":  # the ball 0.3 away inside the fan (even environments) or 1.0 away, out of reach (odd ones)
        state = torch.zeros(3, 6, n, dtype=F64)
        state[2, 0:2] = 0.05 * U(2, n)
        state[0, 0:2] = state[2, 0:2] + torch.where((torch.arange(n) // K) % 2 == 1, 1.0, 0.3) * unit(0.15 + 0.6 * U(n))
        state[1, 0:2] = state[2, 0:2] + 0.2
    elif name == "q":
        state = torch.zeros(5, 6, n, dtype=F64)
        state[0, 0:2], state[1, 0:2] = 0.04 * U(2, n), torch.tensor([[0.0], [-0.5]]) + 0.06 * U(2, n)
        for k in range(3):
            state[2 + k, 0:2] = 0.36 * unit(0.5 + 2.094 * k + 0.3 * U(n)) + 0.04 * U(2, n)
        state[:, 4] = 3 * U(5, n)
    else:
        state, phi = torch.zeros(17, 6, n, dtype=F64), 2 * math.pi * torch.arange(17, dtype=F64)[:, None] / 17
        state[:, 0:2] = (0.5 * unit(phi) + 0.01 * U(2, 17, n)).transpose(0, 1)
        state[:, 4] = phi + math.pi / 2 + math.pi / 17 + 0.1 * U(17, n)
    return state


def rot2(v, th):
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([v[0] * c - v[1] * s, v[0] * s + v[1] * c])


# One target's distances [R, n] for the rays o + t d, and a tag per ray: the sphere's dn / r, the box's winning slab, 0.
def sphere(o, d, tp, trot, G, R, note):
    r, u, lp = f32(G.radius), tp - o, o + d * (R / 2)
    cp = lp - ((lp - tp) * d).sum(0) * d
    dn, ud = norm(tp - cp), (u * d).sum(0)
    note(dn / r - 1, 1.0), note(ud / norm(u), 1.0)
    a = r * r - dn * dn
    dist = norm(cp - o) - torch.sqrt(torch.where(a > 0, a, torch.full_like(a, 1e-8)))
    return torch.where((dn < r) & (ud > 0), dist, torch.full_like(dist, R)), (dn / r).detach()


def box(o, d, tp, trot, G, R, note):
    L, W, p, q = f32(G.length), f32(G.width), rot2(o - tp, -trot), rot2(d, -trot)
    tx1, tx2, ty1, ty2 = (-L / 2 - p[0]) / q[0], (L / 2 - p[0]) / q[0], (-W / 2 - p[1]) / q[1], (W / 2 - p[1]) / q[1]
    ax, ay = torch.minimum(tx1, tx2), torch.minimum(ty1, ty2)
    t0, t1 = torch.maximum(ax, ay), torch.minimum(torch.maximum(tx1, tx2), torch.maximum(ty1, ty2))
    note(t0, max(L, W)), note(t1 - t0, max(L, W)), note(ax - ay, max(L, W))
    dist = norm(o - (rot2(t0 * q + p, trot) + tp))
    slab = torch.where(ax > ay, (tx2 < tx1).to(F64), 2 + (ty2 < ty1).to(F64))
    return torch.where((t1 >= t0) & (t0 > 0), dist, torch.full_like(dist, R)), slab.detach()


def line(o, d, tp, trot, G, R, note):
    L, qo = f32(G.length), o - tp
    rr = L * unit(trot)
    rxs = cross(rr, d)
    tt, uu = cross(qo, d / rxs), cross(qo, rr / rxs)
    note(tt.abs() - 0.5, 1.0), note(uu, L), note(rxs, L)
    miss = (rxs == 0) | (tt > 0.5) | (tt < -0.5) | (uu < 0)
    return torch.where(miss, torch.full_like(uu, R), norm(uu * d)), torch.zeros_like(uu).detach()


def cast(spec, state, notes=None):
    """World.cast_rays for every sensor of ``spec`` in plain torch ops, in the dtype of ``state`` [E, 6, n] -> [n_lidars, max_rays, n].
    ``notes``: per environment the smallest branch quantity over its own scale ("margin": 0 where a sphere wins grazing),
    and per sensor the winner (0: nothing within max_range, 1 + i: target i) and its tag."""
    n, max_rays = state.shape[2], max(S.n_rays for S in spec.lidars)
    margin, rows = torch.full((n,), math.inf, dtype=F64), []

    def note(q, scale):
        if notes is not None:
            margin.copy_(torch.minimum(margin, (q.detach().to(F64) / scale).abs().reshape(-1, n).min(0).values))

    for S in spec.lidars:
        o, R = state[S.entity, 0:2, None], f32(S.max_range)
        d = unit(torch.tensor(S.angles, dtype=state.dtype)[:, None] + state[S.entity, 4][None])
        hits = [(sphere, box, line)[spec.entities[e].shape](o, d, state[e, 0:2, None], state[e, 4][None], spec.entities[e], R, note)
                for e in S.targets]
        dists = torch.stack([torch.full_like(d[0], R)] + [h[0] for h in hits])
        best, win = dists.min(0)
        if notes is not None:
            tag = torch.stack([torch.zeros_like(hits[0][1])] + [h[1] for h in hits]).gather(0, win[None])[0]
            two = dists.detach().topk(2, dim=0, largest=False).values  # (the max_range row is one of the candidates)
            note(torch.where(win > 0, two[1] - two[0], torch.ones_like(best)), R)
            shape = torch.tensor([-1] + [spec.entities[e].shape for e in S.targets])[win]
            margin[((shape == A.SHAPE_SPHERE) & (tag > 0.9)).any(0)] = 0.0
            notes.setdefault("sensors", []).append((win, tag, shape))
        rows.append(torch.cat([best, torch.zeros(max_rays - S.n_rays, n, dtype=state.dtype)]))
    if notes is not None:
        notes["margin"] = margin
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def reference(name, batch):
    spec = build_world(name, batch).spec
    cand, notes = make_inputs(name, batch * K, WORLDS[name][batch]), {}
    cast(spec, cand, notes)
    ok = (notes["margin"] >= 1e-3).reshape(batch, K)
    assert ok.any(1).all(), "an environment has no candidate that meets the conditions on the inputs"
    state = cand[:, :, torch.arange(batch) * K + ok.to(torch.int8).argmax(1)]
    notes, w = {}, [torch.randn(len(spec.lidars), max(S.n_rays for S in spec.lidars), batch, generator=torch.Generator().manual_seed(1), dtype=F64)]
    g64, out64 = grads(lambda s: (cast(spec, s, notes),), [state], w, F64)
    assert notes["margin"].min() >= 1e-3
    wins = notes["sensors"]
    hit = torch.cat([win > 0 for win, _, _ in wins])
    if name == "p":  # even environments hit, odd ones have nothing in reach: every cotangent is exactly 0 there
        assert hit[:, 0::2].any(0).all() and not hit[:, 1::2].any() and not g64[0][:, :, 1::2].any()
    else:
        assert hit.to(F64).mean() >= 0.25
    if name == "q":  # every target wins a ray of at least two sensors, every slab of the box wins somewhere
        for e in range(spec.n_entities):
            assert sum(bool((win == 1 + S.targets.index(e)).any()) for S, (win, _, _) in zip(spec.lidars, wins) if e in S.targets) >= 2
        assert {int(t) for win, tag, shape in wins for t in tag[shape == A.SHAPE_BOX]} == {0, 1, 2, 3}
    g32, _ = grads(lambda s: (cast(spec, s),), [state], w, torch.float32)
    return spec, state, w[0], g64, g32, out64[0]


@pytest.mark.parametrize("name,batch", CASES)
def test_cast_rays_vjp_against_float64_autograd(name, batch):
    from vectorizedmultiagentsimulator_amd import differentiable
    from vectorizedmultiagentsimulator_amd.backend import HipWorld

    spec, state, w, g64, g32, out64 = reference(name, batch)
    hw = HipWorld(spec, batch)
    assert hw.lidar_vjp_supported() is None
    if name == "r":  # more sensors than one run or one round of waves holds
        assert hw.lidar_vjp_plan()["runs"] == 2 and hw.lidar_vjp_plan()["units"] == 17
    s, gw = packed(state, hw.ld).requires_grad_(), packed(w, hw.ld)
    gw[:, :, batch:] = 7.0  # (padding columns of the cotangent are not read)
    out = differentiable.cast_rays(hw, s)
    hw.state.copy_(s.detach())
    assert torch.equal(out.detach(), hw.cast_rays()) and out.data_ptr() != hw.cast_rays().data_ptr()
    torch.testing.assert_close(out[:, :, :batch].detach().cpu().to(F64), out64, atol=1e-5, rtol=1e-5)
    (got,), again = torch.autograd.grad((out * gw).sum(), [s]), hw.cast_rays_vjp(s.detach(), gw)
    assert torch.equal(got, again), "two runs differ"
    others = [e for e in range(spec.n_entities) if all(e != S.entity and e not in S.targets for S in spec.lidars)]
    assert not got[:, :, batch:].any() and not got[:, [2, 3, 5]].any() and not got[others].any()
    bound_and_check([got[:, :, :batch]], g64, g32, f"{name}/{batch}")


def test_make_env_navigation_gradient_through_the_lidar():
    from vectorizedmultiagentsimulator_amd.environment import make_env

    B, n = 65, 3
    env = make_env("navigation", num_envs=B, n_agents=n, grad_enabled=True, seed=3)
    spec, sc = env.world.spec, env.scenario
    ents, goals = [a._index for a in env.agents], [a.goal._index for a in env.agents]
    g = torch.Generator().manual_seed(5)
    U = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1  # noqa: E731
    for k, a in enumerate(env.agents):  # a triangle of side 0.27 whose sides point between two rays: each agent measures both others with two rays
        a.set_pos((0.156 * unit(math.pi / 12 + 2 * math.pi / 3 * k + 0.02 * U(B)) + 0.004 * U(2, B)).T.to(torch.float32).cuda(), None)
        a.pos_shaping = torch.linalg.vector_norm(a.state.pos - a.goal.state.pos, dim=1) * sc.pos_shaping_factor
    state0, ft0 = env.world._state[:, :, :B].detach().cpu().to(F64), env.world._agent_ft[:, :, :B].detach().cpu().to(F64)
    acts = [0.3 * U(n, B, 2) for _ in range(2)]
    wobs = torch.randn(n, B, 6 + sc.n_lidar_rays, generator=g, dtype=F64)
    mult = torch.stack([a.action.u_multiplier_tensor_on("cpu").to(F64) for a in env.agents])[:, None, :]
    rows, notes = [a._agent_index for a in env.agents], {}

    def ref(a1, notes=None):
        state, ft = state0.to(a1.dtype), ft0.to(a1.dtype)
        for a in (a1, acts[1].to(a1.dtype)):
            ft = ft.index_copy(0, torch.tensor(rows), torch.cat([(a * mult.to(a1.dtype)).transpose(1, 2), ft[rows, 2:3]], dim=1))
            state, ft = restate_step(spec, state, ft)
        lidar = f32(sc.lidar_range) - cast(spec, state, notes)[:, : sc.n_lidar_rays]
        obs = torch.cat([state[ents, 0:4], state[ents, 0:2] - state[goals, 0:2], lidar], dim=1)  # [n, 6 + rays, B]
        # the rewards of both steps summed over the agents: the shared shaping differences telescope, the rest is constant
        rew = n * (norm((state0[ents, 0:2] - state0[goals, 0:2]).transpose(0, 1)).to(a1.dtype) - norm((state[ents, 0:2] - state[goals, 0:2]).transpose(0, 1))).sum(0)
        return (obs, rew * f32(sc.pos_shaping_factor))

    w = [wobs.permute(0, 2, 1), torch.ones(B, dtype=F64)]
    g64, _ = grads(lambda a: ref(a, notes), [acts[0]], w, F64)
    assert notes["margin"].min() >= 1e-3 and torch.cat([x[0] > 0 for x in notes["sensors"]]).to(F64).mean() >= 0.25
    g32, _ = grads(ref, [acts[0]], w, torch.float32)
    a1 = acts[0].to(torch.float32).cuda().requires_grad_()
    _, r1, _, _ = env.step(list(a1))
    obs, r2, _, _ = env.step(list(acts[1].to(torch.float32).cuda()))
    loss = (torch.stack(obs) * wobs.to(torch.float32).cuda()).sum() + torch.stack(r1 + r2).sum()
    bound_and_check(torch.autograd.grad(loss, [a1]), g64, g32, "navigation/65 with its LIDAR")
