"""``vmas_world_step_env_checked``: the reference's action asserts as ONE foreign call and TWO launches - the check, then the
step gated on it, which reports the check's verdict to the host itself (``env_gate_report``, csrc/vmas_step_types.h) where a
one-thread marker launch between the two used to.  (The lane-compacted kernel - football - and navigation's kernels keep the marker launch, made
by the same call.)  Only the launch structure changes, so everything here is bitwise: a validated environment against its
``validate_actions=False`` twin for every kernel form that reads the gate, refusals that leave the world untouched, the
attached reference, and the three-call path the entry replaces."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FOOTBALL = dict(n_blue_agents=5, n_red_agents=5, ai_red_agents=False)
TWO_LAUNCHES = 16448  # 257 tiles: the first size beyond one tile per CU - navigation's collision kernel, football's post-step

# id -> (scenario, kwargs, environments, interpreter forced)
FORMS = {
    "balance-100": ("balance", dict(n_agents=4), 100, False),  # the last tile is partial
    "balance-2048": ("balance", dict(n_agents=4), 2048, False),
    "balance-100-interpreter": ("balance", dict(n_agents=4), 100, True),
    "transport-2048": ("transport", {}, 2048, False),
    "navigation-256": ("navigation", dict(n_agents=8), 256, False),
    "football-256": ("football", FOOTBALL, 256, False),  # the lane-compacted kernel
    "navigation-16448": ("navigation", dict(n_agents=8), TWO_LAUNCHES, False),
    "football-16448": ("football", FOOTBALL, TWO_LAUNCHES, False),
}
REFUSAL_FORMS = ["balance-100", "balance-2048", "navigation-16448", "football-16448"]


def _pair(form, seed=2):
    from vectorizedmultiagentsimulator_amd.environment import make_env

    name, kw, B, interpreter = FORMS[form]
    env = make_env(name, num_envs=B, device=DEV, seed=seed, validate_actions=True, **kw)
    twin = make_env(name, num_envs=B, device=DEV, seed=seed, validate_actions=False, **kw)
    for e in (env, twin):
        assert e._one_launch
        if interpreter:
            e.world._get_backend().set_specialized(False)
    assert env._launch.can_gate(env._post.kind) and env._launch.can_check()
    return env, twin


def _actions(env, g):
    return [(torch.rand(env.num_envs, a.action_size, device=DEV, generator=g) * 2 - 1) * a.action.u_range_tensor_on(DEV)
            for a in env.agents]


def _shaping(env, name):
    sc = env.scenario
    if name == "balance":
        return [sc.global_shaping]
    if name == "transport":
        return [getattr(p, n) for p in sc.packages for n in ("global_shaping", "on_goal")]
    if name == "navigation":
        return [a.pos_shaping for a in env.world.agents]
    return [getattr(sc.ball, n) for n in ("pos_shaping_blue", "pos_shaping_red", "pos_shaping_agent_blue", "pos_shaping_agent_red")]


def _same_step(o1, o2, what):
    assert all(torch.equal(x, y) for x, y in zip(o1[0], o2[0])), f"{what}: observations"
    assert all(torch.equal(x, y) for x, y in zip(o1[1], o2[1])), f"{what}: rewards"
    assert torch.equal(o1[2], o2[2]), f"{what}: dones"


@pytest.mark.parametrize("form", list(FORMS))
def test_checked_steps_are_bitwise_the_unvalidated_steps(form):
    env, twin = _pair(form)
    g = torch.Generator(device=DEV).manual_seed(11)
    for t in range(4):
        acts = _actions(env, g)
        _same_step(env.step([a.clone() for a in acts]), twin.step(acts), f"{form} step {t}")
        assert torch.equal(env.world._state, twin.world._state), f"{form} step {t}: state"
    torch.cuda.synchronize()
    assert env.world._get_backend().exact_status() == 0


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("poison,what", [(float("nan"), "NaN"), (1.7, "out of its range")], ids=["nan", "range"])
@pytest.mark.parametrize("form", REFUSAL_FORMS)
def test_a_refused_action_leaves_the_world_untouched(form, poison, what, where):
    name, _, B, _ = FORMS[form]
    env, twin = _pair(form)
    g = torch.Generator(device=DEV).manual_seed(12)
    acts = _actions(env, g)
    _same_step(env.step([a.clone() for a in acts]), twin.step(acts), f"{form}: the step before")
    torch.cuda.synchronize()
    state, steps = env.world._state.clone(), env.steps.clone()
    shaping = [x.clone() for x in _shaping(env, name)]
    good = _actions(env, g)
    bad = [a.clone() for a in good]
    bad[-1][0 if where == "first" else B - 1, 0] = poison  # (B - 1: inside the partial tile where there is one)
    with pytest.raises(AssertionError, match=what):
        env.step(bad)
    torch.cuda.synchronize()
    assert torch.equal(env.world._state, state), "a refused action must not touch the state"
    assert torch.equal(env.steps, steps), "... nor the step counter"
    assert all(torch.equal(x, y) for x, y in zip(_shaping(env, name), shaping)), "... nor the scenario's shaping"
    _same_step(env.step([a.clone() for a in good]), twin.step(good), f"{form}: the step after the refusal")
    assert torch.equal(env.world._state, twin.world._state)
    torch.cuda.synchronize()
    assert env.world._get_backend().exact_status() == 0


def test_a_refusal_among_exact_broad_phase_steps_keeps_the_lazy_slots_clean():
    """tests/test_broad_phase_lazy_gpu.py's gated case through the new entry: a refused launch does not publish, the steps
    behind it still see the batch's words."""
    from vectorizedmultiagentsimulator_amd.environment import make_env

    env = make_env("balance", num_envs=2048, device=DEV, seed=3, n_agents=4)
    assert env.world.exact_broad_phase and env.world._get_backend().exact_form() == 1 and env._launch.can_check()
    twin = make_env("balance", num_envs=2048, device=DEV, seed=3, n_agents=4, exact_broad_phase=True)
    g = torch.Generator(device=DEV).manual_seed(5)
    for k in range(12):
        acts = [(torch.rand(2048, 2, device=DEV, generator=g) * 2 - 1) for _ in env.agents]
        if k == 5:
            bad = [a.clone() for a in acts]
            bad[1][7, 0] = float("nan")
            with pytest.raises(AssertionError, match="NaN"):
                env.step(bad)
        o1, o2 = env.step(acts), twin.step(acts)
        assert torch.equal(torch.stack(o1[0]), torch.stack(o2[0])), f"step {k}"
    assert env.world._get_backend().exact_status() == 0


@pytest.mark.reference
def test_the_attached_reference_steps_through_the_new_entry():
    from oracle import ref
    from vectorizedmultiagentsimulator_amd.adapter import attach

    try:  # (a tree whose byte-compiled reference did not travel with it: the stamp is there, the modules are not)
        ref.import_vmas()
        ref.scenario_class("balance")
    except (ImportError, ValueError) as e:
        pytest.skip(f"the reference is not importable here: {e}")
    a = ref.make_env("balance", num_envs=2048, device="cuda", seed=0)
    b = ref.make_env("balance", num_envs=2048, device="cuda", seed=0)
    ha, hb = attach(a), attach(b, validate_actions=False)  # (default validation: the reference's asserts kept)
    assert ha.fused.one_launch and ha.fused.launch.can_check()
    for ea, eb in zip(a.world.entities, b.world.entities):  # the twin starts where `a` does
        eb.set_pos(ea.state.pos.clone(), batch_index=None)
        eb.set_vel(ea.state.vel.clone(), batch_index=None)
        eb.set_rot(ea.state.rot.clone(), batch_index=None)
        eb.set_ang_vel(ea.state.ang_vel.clone(), batch_index=None)
    b.scenario.global_shaping.copy_(a.scenario.global_shaping)
    calls = [0]
    ha.fused.launch._bind()
    inner = ha.fused.launch._checked_fn

    def counted(*args):
        calls[0] += 1
        return inner(*args)

    ha.fused.launch._checked_fn = counted
    rebind = ha.fused.launch._bind

    def bind_and_wrap():
        rebind()
        ha.fused.launch._checked_fn = counted

    ha.fused.launch._bind = bind_and_wrap
    g = torch.Generator(device=DEV).manual_seed(13)
    for t in range(5):
        acts = [(torch.rand(2048, 2, device=DEV, generator=g) * 2 - 1) for _ in a.agents]
        _same_step(a.step([x.clone() for x in acts]), b.step(acts), f"attached step {t}")
    assert torch.equal(ha.state, hb.state)
    assert calls[0] == 5, "every asserts-kept step is one call of vmas_world_step_env_checked"
    before = ha.state.clone()
    bad = [(torch.rand(2048, 2, device=DEV, generator=g) * 2 - 1) for _ in a.agents]
    bad[0][2047, 1] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        a.step(bad)
    torch.cuda.synchronize()
    assert torch.equal(ha.state, before) and calls[0] == 6 and ha.fused.one_launch
    ha.detach(); hb.detach()


def test_the_three_call_path_still_works():
    """validate_begin -> gated -> validate_end (marker launch between check and step), which Python no longer takes with a
    library that has the new entry: the same outcomes, driven through the ``fused`` helpers."""
    from vectorizedmultiagentsimulator_amd.environment import make_env

    env = make_env("balance", num_envs=256, device=DEV, seed=4, n_agents=4, validate_actions=True)
    twin = make_env("balance", num_envs=256, device=DEV, seed=4, n_agents=4, validate_actions=False)
    g = torch.Generator(device=DEV).manual_seed(14)
    good = _actions(env, g)

    def three_calls(actions):
        env._ingest.prepare(actions)
        seq = env._ingest.validate_begin()
        saved = env._post.save_bound()
        desc, buffers, result = env._post.prepare()
        env._launch.gated(env._post.kind, desc, buffers)
        flags = env._ingest.validate_end(seq)
        if flags:
            env._launch.refused()
            env._post.restore_bound(saved)
        return flags, result

    flags, result = three_calls([a.clone() for a in good])
    assert flags == 0
    _same_step(result, twin.step(good), "three calls, good actions")
    torch.cuda.synchronize()
    state = env.world._state.clone()
    bad = [a.clone() for a in good]
    bad[0][255, 0] = float("nan")
    flags, _ = three_calls(bad)
    torch.cuda.synchronize()
    assert flags == 1 and torch.equal(env.world._state, state)
    nxt = _actions(env, g)
    _same_step(env.step([a.clone() for a in nxt]), twin.step(nxt), "the new entry behind the three-call path")
