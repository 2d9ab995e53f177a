"""LIDAR kernel timing on `navigation` (BASELINE config 4): all 8 agents x 12 rays x 7 targets."""
import os, sys, json
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from vectorizedmultiagentsimulator_amd.environment import make_env
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
env = make_env("navigation", num_envs=B, device="cuda:0", n_agents=8, seed=0, validate_actions=False)
w = env.world
be = w._get_backend()
if os.environ.get("LIDAR_COMPACT"):  # A/B: 0 the plain kernel, 1 the lane-compacted cast
    be.set_lidar_compact(int(os.environ["LIDAR_COMPACT"]))
for _ in range(50 if os.environ.get("MIDGAME", "1") == "1" else 0):  # a typical mid-episode state, not the spawn
    env.step([env.get_random_action(a) for a in env.agents])
import time


def vjp_leg():
    """--vjp: the backward launch (csrc/vmas_lidar_vjp.hip) next to the forward cast on the same states, and torch autograd of a
    float32 restatement of the sphere cast as the comparison: device events around windows of launches, alternating."""
    state, g_out = be.state.clone(), torch.randn_like(be.cast_rays())
    S0 = w.spec.lidars[0]
    ents = torch.tensor([S.entity for S in w.spec.lidars], device="cuda:0")
    tgts = torch.tensor([S.targets for S in w.spec.lidars], device="cuda:0")
    ang, R, r = torch.tensor(S0.angles, device="cuda:0"), S0.max_range, w.spec.entities[S0.entity].radius

    def torch_cast(st):  # [E, 6, ld] -> [8, 12, ld]: core.py:1414-1490 for every (sensor, target, ray), then the min
        o, tp = st[ents, 0:2][:, None, :, None], st[tgts][:, :, 0:2, None]  # [8, 1, 2, 1, ld], [8, 7, 2, 1, ld]
        d = torch.stack([torch.cos(ang), torch.sin(ang)])[None, None, :, :, None]
        u, lp = tp - o, o + d * (R / 2)
        cp = lp - ((lp - tp) * d).sum(2, keepdim=True) * d
        dn = torch.linalg.vector_norm(tp - cp, dim=2)
        a = r * r - dn * dn
        dist = torch.linalg.vector_norm(cp - o, dim=2) - torch.sqrt(torch.where(a > 0, a, torch.full_like(a, 1e-8)))
        dist = torch.where((dn < r) & ((u * d).sum(2) > 0), dist, torch.full_like(dist, R))
        return torch.minimum(dist.min(1).values, torch.full_like(dist[:, 0], R))

    def torch_vjp():
        st = state.detach().requires_grad_()
        torch.autograd.grad((torch_cast(st) * g_out).sum(), [st])

    legs = {"forward_us": (lambda: be.cast_rays(state=state), 100), "vjp_us": (lambda: be.cast_rays_vjp(state, g_out), 100),
            "torch_f32_forward_and_autograd_us": (torch_vjp, 5)}
    assert torch.allclose(torch_cast(state), be.cast_rays(state=state), atol=1e-5)
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.5:
        for fn, _ in legs.values():
            fn()
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(7):
        for k, (fn, n) in legs.items():
            e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / n * 1e3)
    out = {"B": B, "lidar_vjp_plan": be.lidar_vjp_plan(), "lib": os.environ.get("VMAS_HIP_LIB", "")}
    for k, v in times.items():
        v.sort()
        out[k] = {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}
    print(json.dumps(out))


if "--vjp" in sys.argv:
    vjp_leg()
    sys.exit(0)
t_warm = time.perf_counter()
while time.perf_counter() - t_warm < 0.25:  # (the clocks of a just-started process are ramping)
    be.cast_rays()
    torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 200
e0.record()
for _ in range(n):
    be.cast_rays()
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) / n * 1e3
rays = B * 8 * 12
print(json.dumps({"B": B, "compact": be.lidar_compact, "lidar_us": us, "rays_per_s": rays / (us * 1e-6), "ray_tests_per_s": rays * 7 / (us * 1e-6),
                  "bytes_per_env": 8 * 12 + 8 * 12 * 4, "GBps": B * (96 + 384) / (us * 1e-6) / 1e9}))
# physics step of the same world, and a full Environment.step for the Amdahl picture
forces = torch.zeros(1, *be.agent_ft.shape, device="cuda:0")
e0.record()
be.step_n(n)
e1.record(); torch.cuda.synchronize()
print(json.dumps({"world_step_us": e0.elapsed_time(e1) / n * 1e3, "lanes": be.lanes_per_env}))
acts = [env.get_random_action(a) for a in env.agents]
for _ in range(3): env.step(acts)
torch.cuda.synchronize()
import time
t0 = time.perf_counter()
for _ in range(20): env.step(acts)
torch.cuda.synchronize()
print(json.dumps({"env_step_ms": (time.perf_counter() - t0) / 20 * 1e3, "env_steps_per_s": B * 20 / (time.perf_counter() - t0)}))
