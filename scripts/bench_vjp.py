"""Time of the backward kernel of World.step next to the forward kernel's, and torch autograd of the float32 restatement of
the same step (tests/test_step_vjp_gpu.py, tests/test_step_vjp_shapes_gpu.py) on the same GPU: N spheres x B environments,
substeps 1, or ``--world transport``: 4 agents and 1 package with every agent touching the package.  Device events around
many launches, after a warm-up; forward and backward windows alternate.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_step_vjp_gpu  # noqa: E402
import test_step_vjp_shapes_gpu  # noqa: E402
from vectorizedmultiagentsimulator_amd.backend import HipWorld  # noqa: E402
from vectorizedmultiagentsimulator_amd.core import Agent, Sphere, World  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", choices=("spheres", "transport"), default="spheres")
    ap.add_argument("--spheres", type=int, default=8)
    ap.add_argument("--envs", type=int, default=None, help="default: 65 536 (spheres), 16 384 (transport)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    a.envs = a.envs or (65536 if a.world == "spheres" else 16384)
    torch.manual_seed(0)
    if a.world == "spheres":
        restate = test_step_vjp_gpu.restate
        w = World(a.envs, "cpu", substeps=1)
        for i in range(a.spheres):
            w.add_agent(Agent(f"agent_{i}", shape=Sphere(0.1)))
        hw = HipWorld(w.spec, a.envs)
        state0 = torch.zeros_like(hw.state)
        state0[:, 0:2] = torch.rand_like(state0[:, 0:2]) * 1.2 - 0.6  # 8 discs of radius 0.1 in a 1.2 x 1.2 box: contacts in most environments
    else:  # the scenario's world (goal, package, 4 agents): an agent on each edge of the package, 0.2 - 3 mm inside its reach
        from vectorizedmultiagentsimulator_amd.scenarios.transport import Scenario

        restate = test_step_vjp_shapes_gpu.restate
        w = Scenario().env_make_world(a.envs, "cpu", n_agents=4)
        hw = HipWorld(w.spec, a.envs)
        state0 = torch.zeros_like(hw.state)
        state0[:2, 0:2] = torch.rand_like(state0[:2, 0:2]) * 1.6 - 0.8
        reach = 0.075 + (0.03 + 4.0 / 6e2) - 2e-4 * 15.0 ** torch.rand(4, 1, hw.ld, device="cuda")
        along = torch.rand(4, 1, hw.ld, device="cuda") * 0.08 - 0.04
        sign = torch.tensor([1.0, -1.0, 1.0, -1.0], device="cuda")[:, None, None]
        offset = torch.cat([sign * reach, along], dim=1)
        offset[2:] = offset[2:].flip(1)
        state0[2:, 0:2] = state0[1:2, 0:2] + offset
    state0[:, 2:4] = torch.rand_like(state0[:, 2:4]) * 0.6 - 0.3
    ft0 = torch.rand_like(hw.agent_ft) - 0.5
    g_state, g_ft = torch.randn_like(state0), torch.randn_like(ft0)
    out_s, out_f = torch.zeros_like(state0), torch.zeros_like(ft0)
    # (the forward steps in place: every launch of a window gets its own copy of the start, so that all of them see its contacts)
    copies = [(state0.clone(), ft0.clone()) for _ in range(a.launches)]
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream

    def forward(i):
        hw.lib.vmas_world_step(hw._h, p(copies[i][0]), p(copies[i][1]), hw.ld, None, stream)

    def backward(i):
        hw.lib.vmas_world_step_vjp(hw._h, p(state0), p(ft0), hw.ld, p(g_state), p(g_ft), p(out_s), p(out_f), stream)

    def window(fn):
        for s, f in copies:
            s.copy_(state0), f.copy_(ft0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.launches):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches

    for fn in (forward, backward):
        window(fn)
    t = {"forward": [], "backward": []}
    for _ in range(a.windows):
        t["forward"].append(window(forward))
        t["backward"].append(window(backward))
    spec, B = hw.spec, a.envs
    sa, fa = state0[:, :, :B].clone().requires_grad_(), ft0[:, :, :B].clone().requires_grad_()
    auto = []
    for i in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = restate(spec, sa, fa)
        torch.autograd.grad((o[0] * g_state[:, :, :B]).sum() + (o[1] * g_ft[:, :, :B]).sum(), [sa, fa])
        torch.cuda.synchronize()
        if i >= 3:
            auto.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps({"world": a.world, "entities": spec.n_entities, "pairs": len(spec.pairs), "envs": B, "substeps": spec.substeps, "launches_per_window": a.launches,
                      "forward_us": statistics.median(t["forward"]), "forward_us_minmax": [min(t["forward"]), max(t["forward"])],
                      "backward_us": statistics.median(t["backward"]), "backward_us_minmax": [min(t["backward"]), max(t["backward"])],
                      "torch_autograd_float32_forward_plus_backward_us": statistics.median(auto)}))


if __name__ == "__main__":
    main()
