"""The backward kernel of World.step (csrc/vmas_vjp.hip) against torch autograd of a plain float64 restatement of the
sphere-world step on the CPU.  The bound is 4 x the error the SAME restatement makes in float32, computed at run time
(figures seen on one MI355X: DESIGN.md 3.4b)."""
import functools

import numpy as np
import pytest
import torch

from vectorizedmultiagentsimulator_amd import _abi as A
from vectorizedmultiagentsimulator_amd.core import Agent, Landmark, Sphere, World

pytestmark = pytest.mark.gpu
F64 = torch.float64
CLAMPS = dict(max_speed=0.5, v_range=0.4, max_f=0.8, f_range=0.6, max_t=0.5, t_range=0.4, gravity=(0.0, -0.3))
#: world -> (designated contact pairs, seed per batch size: chosen on the CPU so that the branch condition below holds)
WORLDS = {"a": ([(0, 1)], {1: 0, 64: 0, 65: 0, 130: 0}), "b": ([(0, 2), (3, 4)], {63: 4, 130: 1}),
          "c": ([(2 * i, 2 * i + 1) for i in range(8)], {63: 27, 130: 36})}
CASES = [(n, b) for n, (_, seeds) in WORLDS.items() for b in seeds]


def build_world(name, batch, device="cpu", **kw):
    """(a) 2 spheres; (b) 3 clamped agents, an immovable and a non-collidable landmark, gravity, bounds; (c) 17 spheres."""
    bounds = dict(x_semidim=1.0, y_semidim=1.0, gravity=(0.1, -0.2)) if name == "b" else {}
    w = World(batch, device, substeps={"a": 1, "b": 2, "c": 5}[name], **bounds, **kw)
    if name == "b":
        w.add_landmark(Landmark("wall", shape=Sphere(0.05)))
        w.add_landmark(Landmark("mark", collide=False))
    for i in range(4 if name == "c" else 0):
        w.add_landmark(Landmark(f"ball_{i}", movable=True, shape=Sphere(0.05)))
    for i in range({"a": 2, "b": 3, "c": 13}[name]):
        w.add_agent(Agent(f"agent_{i}", shape=Sphere(0.1), **(CLAMPS if name == "b" else {})))
    return w


def d_min(spec, a, b):
    return float(np.float32(spec.entities[a].radius) + np.float32(spec.entities[b].radius))


def make_inputs(spec, contacts, batch, seed, clamps):
    """Seeded (state [E, 6, B], agent_ft [A, 3, B]) in float64: clusters 0.7 apart, contact pairs at dist = dmin - delta with
    delta log-uniform over [2e-4, 3e-3]; with clamps, the environment index decides which clamp is clearly on / off."""
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    unit = lambda th: torch.stack([torch.cos(th), torch.sin(th)])  # noqa: E731
    E, env = spec.n_entities, torch.arange(batch)
    state, ft = torch.zeros(E, 6, batch, dtype=F64), torch.zeros(max(spec.n_agents, 1), 3, batch, dtype=F64)
    second = {b: a for a, b in contacts}
    heads = [e for e in range(E) if e not in second][::-1]
    for i, e in enumerate(heads):
        state[e, 0:2] = torch.tensor([[0.8 - 0.7 * (i % 3)], [-0.6 + 0.7 * (i // 3)]]) + 0.06 * U(2, batch) - 0.03
    for b, a in second.items():
        delta = 2e-4 * 15.0 ** U(batch)
        state[b, 0:2] = state[a, 0:2] + (d_min(spec, a, b) - delta) * unit(6.283 * U(batch))
    if clamps:  # whole environments pushed over the x / y bound
        state[:, 0] += 0.75 * (env % 4 == 3)
        state[:, 1] -= 0.75 * (env % 4 == 2)
    speed = torch.where(env % 2 == 1, 1.0, 0.4) if clamps else torch.full((batch,), 0.3)
    force = torch.where((env // 2) % 2 == 1, 1.2, 0.4) if clamps else torch.full((batch,), 0.5)
    torque = torch.where((env // 4) % 2 == 1, 1.0, 0.3) if clamps else torch.full((batch,), 0.5)
    for e, D in enumerate(spec.entities):
        state[e, 2:4] = speed * (0.9 + 0.2 * U(batch)) * unit(6.283 * U(batch)) * bool(D.flags & A.F_MOVABLE)
        state[e, 4], state[e, 5] = 6 * U(batch) - 3, 2 * U(batch) - 1
        if D.agent_index >= 0:
            ft[D.agent_index, 0:2] = force * (0.9 + 0.2 * U(batch)) * unit(6.283 * U(batch))
            ft[D.agent_index, 2] = torque * (0.9 + 0.2 * U(batch)) * torch.sign(U(batch) - 0.5)
    return state, ft


def restate(spec, state, ft, margins=None):
    """World.step of a sphere-only world in plain torch ops, in the dtype of ``state``.  ``margins``: collects every branch
    quantity divided by its own scale."""
    note = (lambda q, s: margins.append((q / s).detach().abs().min().item())) if margins is not None else (lambda q, s: None)
    norm = lambda t: torch.linalg.vector_norm(t, dim=0)  # noqa: E731
    f32 = lambda x: float(np.float32(x))  # noqa: E731

    def clamp_norm(t, m):
        n = norm(t)
        note(n - m, m)
        return torch.where(n > m, t / n * m, t)

    def clamp(t, m):
        note(t.abs() - m, m)
        return t.clamp(-m, m)

    dt, k, c, S = f32(spec.sub_dt), f32(spec.contact_margin), f32(spec.collision_force), spec.substeps
    ents = spec.entities
    pos, vel = [state[e, 0:2] for e in range(len(ents))], [state[e, 2:4] for e in range(len(ents))]
    rot, av = [state[e, 4] for e in range(len(ents))], [state[e, 5] for e in range(len(ents))]
    base, Tq, ft_out = [], [], [r for r in ft]
    for e, D in enumerate(ents):
        F, T, fl = torch.zeros_like(pos[e]), torch.zeros_like(rot[e]), D.flags
        if fl & A.F_AGENT:
            f, t = ft[D.agent_index, 0:2], ft[D.agent_index, 2]
            if fl & A.F_MOVABLE:
                f = clamp_norm(f, f32(D.max_f)) if fl & A.F_MAX_F else f
                F = f = clamp(f, f32(D.f_range)) if fl & A.F_F_RANGE else f
            if fl & A.F_ROTATABLE:
                t = clamp_norm(t[None], f32(D.max_t))[0] if fl & A.F_MAX_T else t
                T = t = clamp(t, f32(D.t_range)) if fl & A.F_T_RANGE else t
            ft_out[D.agent_index] = torch.cat([f, t[None]])
        if fl & A.F_MOVABLE:
            G = torch.tensor(spec.gravity, dtype=state.dtype, device=state.device) * bool(spec.has_gravity)
            G = G + torch.tensor(D.gravity, dtype=state.dtype, device=state.device) * bool(fl & A.F_GRAVITY)
            F = F + f32(D.mass) * G[:, None]
        base.append(F)
        Tq.append(T)
    for s in range(S):
        Fs = list(base)
        for P in spec.pairs:
            d = pos[P.a] - pos[P.b]
            dist, dm = norm(d), d_min(spec, P.a, P.b)
            note(dist - dm, dm)
            f = c * d / dist * (k * torch.logaddexp(torch.zeros_like(dist), (dm - dist) / k))
            f = torch.where((dist < 1e-6) | (dist > dm), torch.zeros_like(f), f)
            Fs[P.a], Fs[P.b] = Fs[P.a] + f, Fs[P.b] - f
        for e, D in enumerate(ents):
            drag = f32(D.one_minus_drag) if s == 0 else 1.0
            if D.flags & A.F_MOVABLE:
                v = vel[e] * drag + Fs[e] / f32(D.mass) * dt
                v = clamp_norm(v, f32(D.max_speed)) if D.flags & A.F_MAX_SPEED else v
                v = clamp(v, f32(D.v_range)) if D.flags & A.F_V_RANGE else v
                p = pos[e] + v * dt
                p = torch.stack([p[i] if m is None else clamp(p[i], m) for i, m in enumerate((spec.x_semidim, spec.y_semidim))])
                pos[e], vel[e] = p, v
            if D.flags & A.F_ROTATABLE:
                av[e] = av[e] * drag + Tq[e] / f32(D.inertia) * dt
                rot[e] = rot[e] + av[e] * dt
    return torch.stack([torch.cat([pos[e], vel[e], rot[e][None], av[e][None]]) for e in range(len(ents))]), torch.stack(ft_out)


def grads(fn, leaves, weights, dtype):
    """d sum(w * out) / d leaves of ``fn`` run in ``dtype``, and the outputs."""
    leaves = [t.detach().to(dtype).requires_grad_() for t in leaves]
    outs = fn(*leaves)
    g = torch.autograd.grad(sum((o * w.to(dtype)).sum() for o, w in zip(outs, weights)), leaves)
    return [x.to(F64) for x in g], [o.detach() for o in outs]


def bound_and_check(got, g64, g32, what):
    """|got - g64| / max |g64| <= 4 x the same figure of the float32 restatement, per tensor; every entry compared."""
    for i, (x, r64, r32) in enumerate(zip(got, g64, g32)):
        scale = r64.abs().max().item()
        err, ref_err = (x.cpu().to(F64) - r64).abs().max().item() / scale, (r32 - r64).abs().max().item() / scale
        print(f"{what}[{i}]: HIP {err:.3e}  float32 restatement {ref_err:.3e}  scale {scale:.3e}")
        assert err <= 4 * ref_err, (what, i, err, ref_err)


@functools.lru_cache(maxsize=None)
def reference(name, batch, with_gft):
    spec = build_world(name, batch).spec
    state, ft = make_inputs(spec, WORLDS[name][0], batch, WORLDS[name][1][batch], name == "b")
    g = torch.Generator().manual_seed(1)
    w = [torch.randn(state.shape, generator=g, dtype=F64), torch.randn(ft.shape, generator=g, dtype=F64) * with_gft]
    margins = []
    g64, out64 = grads(lambda s, f: restate(spec, s, f, margins), [state, ft], w, F64)
    assert min(margins) >= 1e-4, f"a branch quantity is within 1e-4 of its kink: {min(margins):.2e}"
    g32, _ = grads(lambda s, f: restate(spec, s, f), [state, ft], w, torch.float32)
    return spec, state, ft, w, g64, g32, out64


def packed(t, ld):
    out = torch.zeros(*t.shape[:2], ld, dtype=torch.float32, device="cuda")
    out[:, :, : t.shape[2]] = t.to(torch.float32)
    return out


@pytest.mark.parametrize("with_gft", [True, False])
@pytest.mark.parametrize("name,batch", CASES)
def test_step_vjp_against_float64_autograd(name, batch, with_gft):
    from vectorizedmultiagentsimulator_amd.backend import HipWorld

    spec, state, ft, w, g64, g32, out64 = reference(name, batch, with_gft)
    hw = HipWorld(spec, batch)
    assert hw.vjp_supported() is None
    s_in, f_in = packed(state, hw.ld), packed(ft, hw.ld)
    s_out, f_out = s_in.clone(), f_in.clone()
    hw.step(state=s_out, agent_ft=f_out)  # the restatement's forward is the validated kernel's, to 1e-5
    for got, want in ((s_out, out64[0]), (f_out, out64[1])):
        torch.testing.assert_close(got[:, :, :batch].cpu().to(F64), want, atol=1e-5, rtol=1e-5)
    run = lambda: hw.step_vjp(s_in, f_in, packed(w[0], hw.ld), packed(w[1], hw.ld) if with_gft else None)  # noqa: E731
    got, again = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(got, again)), "two runs differ"
    assert all(not x[:, :, batch:].any() for x in got), "padding columns were written"
    bound_and_check([x[:, :, :batch] for x in got], g64, g32, f"{name}/{batch}")


def chain_b(step, spec, state, ft, forces, vel0, moved_to):
    """Three steps of (b): velocities and every step's forces from leaves, torques from the inputs, entity 4 re-placed after step 1."""
    state = torch.cat([state[:, 0:2], vel0, state[:, 4:6]], dim=1)
    for i in range(3):
        state, _ = step(state, torch.cat([forces, ft[:, 2:3]], dim=1))
        if i == 0:
            state = torch.cat([state[:4], torch.cat([moved_to.to(state.dtype), state[4, 2:6]])[None]])
    return state[:, 0:2], state[:, 4]


def test_three_chained_world_steps_and_the_forward_under_grad():
    B, contacts = 63, WORLDS["b"][0]
    spec = build_world("b", B).spec
    state, ft = make_inputs(spec, contacts, B, WORLDS["b"][1][B], True)
    moved_to = torch.tensor([[-0.5], [0.6]], dtype=F64) + 0.001 * torch.arange(B, dtype=F64)
    g = torch.Generator().manual_seed(2)
    w = [torch.randn(5, 2, B, generator=g, dtype=F64), torch.randn(5, B, generator=g, dtype=F64)]
    margins, leaves = [], [ft[:, 0:2], state[:, 2:4]]
    ref = lambda m: (lambda F, v: chain_b(lambda s, f: restate(spec, s, f, m), spec, state.to(F.dtype), ft.to(F.dtype), F, v, moved_to))  # noqa: E731
    g64, _ = grads(ref(margins), leaves, w, F64)
    assert min(margins) >= 1e-4, f"a branch quantity is within 1e-4 of its kink: {min(margins):.2e}"
    g32, _ = grads(ref(None), leaves, w, torch.float32)
    F = ft[:, 0:2].to(torch.float32).cuda().requires_grad_()
    v0 = state[:, 2:4].to(torch.float32).cuda().requires_grad_()
    for grad in (False, True):  # the same three steps without the tape first: the forward under grad_enabled is bitwise that one
        with torch.set_grad_enabled(grad):
            world = build_world("b", B, "cuda", grad_enabled=grad)
            world.reset(None)
            for e, ent in enumerate(world.entities):
                ent.set_pos(state[e, 0:2].T, None), ent.set_rot(state[e, 4:5].T, None), ent.set_ang_vel(state[e, 5:6].T, None)
                ent.state.vel = v0[e].T
            for i in range(3):
                for a, agent in enumerate(world.agents):
                    agent.state.force, agent.state.torque = F[a].T, ft[a, 2:3].T
                world.step()
                if i == 0:
                    world.entities[4].set_pos(moved_to.T, None)
        if not grad:
            plain = world._state.clone(), world._agent_ft.clone()
    assert torch.equal(world._state.detach(), plain[0]) and torch.equal(world._agent_ft.detach(), plain[1])
    pos = torch.stack([e.state.pos.T for e in world.entities])
    rot = torch.stack([e.state.rot[:, 0] for e in world.entities])
    got = torch.autograd.grad((pos * w[0].cuda()).sum() + (rot * w[1].cuda()).sum(), [F, v0])
    bound_and_check(got, g64, g32, "chained b/63")


def test_make_env_navigation_gradient_of_observations():
    from vectorizedmultiagentsimulator_amd.environment import make_env

    B = 65
    env = make_env("navigation", num_envs=B, n_agents=3, collisions=False, grad_enabled=True, seed=3)
    spec = env.world.spec
    state0, ft0 = env.world._state[:, :, :B].detach().cpu().to(F64), env.world._agent_ft[:, :, :B].detach().cpu().to(F64)
    g = torch.Generator().manual_seed(4)
    acts = [torch.rand(3, B, 2, generator=g, dtype=F64) * 1.6 - 0.8 for _ in range(2)]
    mult = torch.stack([a.action.u_multiplier_tensor_on("cpu").to(F64) for a in env.agents])[:, None, :]
    rows, ents = [a._agent_index for a in env.agents], [a._index for a in env.agents]

    def ref(a1):
        state, ft = state0.to(a1.dtype), ft0.to(a1.dtype)
        for a in (a1, acts[1].to(a1.dtype)):
            ft = ft.index_copy(0, torch.tensor(rows), torch.cat([(a * mult.to(a1.dtype)).transpose(1, 2), ft[rows, 2:3]], dim=1))
            state, ft = restate(spec, state, ft)
        return (state[ents, 0:4],)

    w = [torch.ones(3, 4, B, dtype=F64)]
    g64, _ = grads(ref, [acts[0]], w, F64)
    g32, _ = grads(ref, [acts[0]], w, torch.float32)
    a1 = acts[0].to(torch.float32).cuda().requires_grad_()
    env.step(list(a1))
    obs, _, _, _ = env.step(list(acts[1].to(torch.float32).cuda().requires_grad_()))
    got = torch.autograd.grad(sum(o[:, :4].sum() for o in obs), [a1])
    bound_and_check(got, g64, g32, "navigation/65")


def test_refusals_name_the_reason():
    from golden_util import load
    from vectorizedmultiagentsimulator_amd.backend import HipWorld
    from vectorizedmultiagentsimulator_amd.scenarios.balance import Scenario

    why = HipWorld(load("balance_n4").spec, 8).vjp_supported()
    assert why is not None and "pair" in why and "sphere-sphere" in why
    world = Scenario().env_make_world(8, "cuda:0", n_agents=4)
    world.grad_enabled = True
    world.reset(None)
    with pytest.raises(NotImplementedError, match="sphere-sphere"):
        world.step()
