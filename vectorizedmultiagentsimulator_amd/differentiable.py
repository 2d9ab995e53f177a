"""``World.step`` on the autograd tape: the forward is the HIP step kernel, the backward ONE launch of the backward
kernel (csrc/vmas_vjp.hip through ``HipWorld.step_vjp``) - no chain of small tensor ops, no tape of them.

Served: worlds whose pairs are sphere-sphere, line-sphere or box-sphere (``HipWorld.vjp_supported()``; DESIGN.md
"Backward of World.step").  First order only: the backward is ``once_differentiable``.

With a line-sphere or box-sphere pair the step that is differentiated is the per-environment one (``exact=False``): past
a line's tip or a box's corner such a pair's force is non-zero where the bounding circles do not overlap, and there the
reference's batch-global rule depends on the other environments of the batch, which a backward without communication
between tiles cannot reproduce.  ``exact=True`` is refused for these worlds.

``World.cast_rays`` is on the tape the same way (``cast_rays`` below): the forward is the LIDAR kernel, the backward ONE
launch of csrc/vmas_lidar_vjp.hip through ``HipWorld.cast_rays_vjp``.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _abi as A

EXACT_REFUSAL = ("the backward kernel differentiates the per-environment step: a world with a line-sphere or box-sphere pair "
                 "cannot be stepped with the batch-global broad phase (exact_broad_phase=True) under grad_enabled")


def has_shape_pairs(spec) -> bool:
    """True if a statically collidable pair of ``spec`` is line-sphere or box-sphere."""
    return any(p.type in (A.PAIR_LS, A.PAIR_BS) for p in spec.pairs)


def planning_refusal(spec):
    """Why the backward kernel refuses ``spec`` (None: it does not), asked of a planning world: no GPU work."""
    import ctypes as C

    for i, e in enumerate(spec.entities):
        if e.per_env_gravity:
            return f"vmas_world_step_vjp: entity {i} has a per-environment gravity tensor, which the backward kernel does not serve"
    lib, desc, h = A.load_library(), spec.to_ctypes(), C.c_void_p()
    if lib.vmas_world_create(C.byref(desc.world), 1, -1, C.byref(h)) != 0:
        return A.last_error()
    why = None if lib.vmas_world_step_vjp_check(h) == 0 else A.last_error()
    lib.vmas_world_destroy(h)
    return why


class _WorldStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hw, exact, state, agent_ft):
        # the inputs stay as they are (they are what the backward re-runs the step from); clones are stepped in place
        out_state = state.clone(memory_format=torch.contiguous_format)
        out_ft = agent_ft.clone(memory_format=torch.contiguous_format)
        hw.step(state=out_state, agent_ft=out_ft, exact=exact)
        ctx.hw = hw
        ctx.save_for_backward(state, agent_ft)
        return out_state, out_ft

    @staticmethod
    @once_differentiable
    def backward(ctx, g_state, g_ft):
        state, agent_ft = ctx.saved_tensors
        g_state_in, g_ft_in = ctx.hw.step_vjp(state.contiguous(), agent_ft.contiguous(), g_state, g_ft)
        return None, None, g_state_in, g_ft_in


def world_step(hw, state: torch.Tensor, agent_ft: torch.Tensor, exact: bool = False):
    """One ``World.step()`` of ``hw`` (a ``HipWorld``) from the packed ``state`` [E, 6, ld] / ``agent_ft`` [A, 3, ld] ->
    ``(state', agent_ft')``, fresh tensors that autograd differentiates with respect to both inputs.  ``agent_ft'`` is
    the force buffer as the step leaves it (clamped where agents have max_f / f_range / max_t / t_range).  ``exact``:
    as ``HipWorld.step``.  For a world of sphere-sphere pairs only it changes nothing (such a pair's force is exactly 0
    wherever the bounding circles do not overlap); with a line-sphere or box-sphere pair it raises ``NotImplementedError``."""
    why = hw.vjp_supported()
    if why is not None:
        raise NotImplementedError(why)
    if exact and has_shape_pairs(hw.spec):
        raise NotImplementedError(EXACT_REFUSAL)
    return _WorldStep.apply(hw, bool(exact), state, agent_ft)


class _CastRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hw, state):
        state = state.contiguous()
        # a fresh tensor per cast: the backend's re-used output buffer would be overwritten under an earlier tape
        out = torch.zeros(len(hw.spec.lidars), hw.cdesc.max_rays, hw.ld, device=state.device, dtype=torch.float32)
        hw.cast_rays(state=state, out=out)
        ctx.hw = hw
        ctx.save_for_backward(state)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        (state,) = ctx.saved_tensors
        return None, ctx.hw.cast_rays_vjp(state, g_out)


def cast_rays(hw, state: torch.Tensor) -> torch.Tensor:
    """``World.cast_rays`` for every registered Lidar of ``hw`` (a ``HipWorld``) from the packed ``state`` [E, 6, ld] ->
    [n_lidars, max_rays, ld], a fresh tensor that autograd differentiates with respect to the positions and rotations in
    ``state``: a ray's cotangent goes to the one target that gave its minimum, and nowhere when nothing is within
    ``max_range``.  Raises ``NotImplementedError`` with the reason when the sensor set is refused."""
    why = hw.lidar_vjp_supported()
    if why is not None:
        raise NotImplementedError(why)
    return _CastRays.apply(hw, state)
