"""CPU tests of the recurrent policies with a feed-forward critic (enable_critic_lstm=False; include/reinfocus_hip.h, "lstm
critic"), under both heads: the numpy twins (lstm.lstm_numpy, lstm_sde.lstm_sde_numpy, lstm_learner.lstm_update_numpy with a
spec of this mode) against the host build of the kernels' own headers (tests/lstmcriticcheck) as bytes; the packing; that the
value path ignores state and episode starts and the update the vf half of lstm_states; the meaning against torch on the CPU
in float64 (torch.nn.LSTM cells stepped per row for the actor, torch.nn.Linear for `critic`, autograd, clip_grad_norm_,
Adam); the binding.

The float64 comparison of a development run (printed by the test; profiles/lstm_critic.md records it), as twin / torch
float32, each the largest distance from torch float64 (head: the logits, or the mean with the Gaussian head):
    categorical (4, 16, relu):  head 1.17e-07 / 1.18e-07; values 2.09e-07 / 2.33e-07; grad 4.31e-08 / 3.43e-08;
                                after 1 update 5.72e-08 / 5.72e-08; after 10 updates 1.98e-07 / 1.98e-07
    categorical (7, 65, tanh):  head 2.65e-07 / 1.85e-07; values 3.27e-07 / 1.16e-07; grad 1.04e-07 / 6.44e-08;
                                after 1 update 5.86e-08 / 5.86e-08; after 10 updates 2.61e-07 / 2.61e-07
    sde (4, 16, relu):          head 1.32e-07 / 5.28e-08; values 2.49e-07 / 1.28e-07; grad 1.33e-07 / 7.39e-08;
                                after 1 update 5.70e-08 / 5.70e-08; after 10 updates 2.87e-07 / 2.87e-07
    sde (7, 65, tanh):          head 1.80e-07 / 1.50e-07; values 5.84e-07 / 2.10e-07; grad 1.07e-07 / 6.64e-08;
                                after 1 update 5.77e-08 / 5.77e-08; after 10 updates 2.99e-07 / 2.99e-07
The largest ratio is 2.83 (values, (7, 65, tanh)).  Leaving the critic layer out moves torch's float64 gradient of
critic.weight by 2.8e-02 .. 1.6e-01, against bounds of 1.4e-07 .. 3.0e-07.
"""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import learner, lstm, lstm_learner, lstm_sde, policy
from tests import lstm_critic_io_cases as cases
from tests import lstm_io_cases as lstm_cases
from tests import lstm_sde_io_cases as lstm_sde_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits
NETWORK_IDS = ["-".join(str(v) for v in network) for network in cases.NETWORKS]


@pytest.fixture(scope="module")
def hostcheck():
    return cases.hostcheck()


def same_dicts(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        if want[key] is None:
            assert got[key] is None, f"{what}: {key}"
        else:
            assert bits(got[key]) == bits(want[key]), f"{what}: {key} differ"


# ---- 1: the twins against the host build --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=NETWORK_IDS)
@pytest.mark.parametrize("head", cases.HEADS)
def test_forward_of_the_header_equals_the_twin(head, index, n, hostcheck):
    """A chain of steps on hostile inputs (+-0, +-inf, subnormals and NaN among the observations and the pi state, start
    bytes 0, 1, 2 and 255, NaN-led final_obs rows, the vf half of the state NaN throughout), sampled and deterministic, then
    a values-only call: every output and the stored state as bytes.  n: one environment, a tile, one past it, ragged."""
    spec, params, obs, final_obs, starts, state = cases.chain_inputs(head, index, n)
    assert hostcheck.lcc_params_size(ctypes.byref(cases.critic_desc(spec)), int(head == "sde")) == spec.size
    for mode in ("sampled", "deterministic"):
        want = cases.wanted_chain(head, index, n, mode)
        _, theta = cases.chain_noise(head, index, n, mode)
        bit_generator = cases.policy_cases.generator_at(0)[0]
        current = state
        for s in range(cases.STEPS):
            gen = policy.generator_words(bit_generator) if mode == "sampled" and head == "categorical" else None
            got = cases.host_forward(hostcheck, head, spec, params, obs[s], starts[s], current, final_obs[s], gen, theta,
                                     mode == "deterministic")
            bit_generator.advance(n)
            same_dicts(got, want[s], f"{mode}, step {s}")
            assert bits(got["state"][0]) == bits(got["state"][1]), "the halves of the stored state differ"
            current = got["state"]
    only = cases.twin_forward(head, spec, params, obs[0], starts[0], state, final_obs[0], None, None, True, values_only=True)
    got = cases.host_forward(hostcheck, head, spec, params, obs[0], starts[0], state, final_obs[0], None, None, True,
                             values_only=True)
    for key in ("values", "final_values"):
        assert bits(got[key]) == bits(only[key]) == bits(cases.wanted_chain(head, index, n, "deterministic")[0][key]), key
    assert only["state"] is None


@pytest.mark.parametrize("index", cases.GPU_NETWORKS, ids=[NETWORK_IDS[i] for i in cases.GPU_NETWORKS])
@pytest.mark.parametrize("head", cases.HEADS)
def test_update_of_the_header_equals_the_twin(head, index, hostcheck):
    """Three chained updates with changing hyper-parameters on every sequence layout of lstm_learner_io_cases.LAYOUTS (the
    network with every limit at B <= 2), the vf half of lstm_states NaN throughout: parameters, optimizer state, stats and
    the gradient as bytes."""
    for name in cases.layouts_of(index):
        spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(head, index, name)
        want = cases.twin_updates(head, index, name)
        state = learner.fresh_state(spec)
        assert hostcheck.lcc_state_size(ctypes.byref(cases.critic_desc(spec)), int(head == "sde")) == 4 * state.size
        for update in range(cases.UPDATES):
            got = cases.host_update(hostcheck, head, spec, params, state, batch, starts, states, n_steps, num_envs, first,
                                    count, cases.hyper_of(update))
            for what, x, y in zip(("params", "state", "stats", "gradient"), got, want[update]):
                assert bits(x) == bits(y), f"{name}, update {update}: {what} differ"
            params, state = got[0], got[1]
        assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()
        assert all(stats[7] == 0 for _, _, stats, _ in want) and bits(want[-1][0]) != bits(want[0][0])


LIMIT_CASES = [(index, name) for index in cases.GPU_NETWORKS for name in cases.limit_layouts_of(index)]


@pytest.mark.parametrize("index,name", LIMIT_CASES, ids=[f"{cases.NETWORKS[i][1]}-{name}" for i, name in LIMIT_CASES])
@pytest.mark.parametrize("head", cases.HEADS)
def test_update_of_the_header_equals_the_twin_at_the_limits(head, index, name, hostcheck):
    """The same on the limit layouts of tests/lstm_learner_io_cases.py (whose CPU test asserts their sequence lengths):
    tuned and depth on both networks below the limits, wave (B = 1024 and 513) on ppo_lstm_tuned.yml's, one 17-row sequence
    on the network with every limit."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(head, index, name)
    want = cases.twin_updates(head, index, name)
    state = learner.fresh_state(spec)
    for update in range(cases.UPDATES):
        got = cases.host_update(hostcheck, head, spec, params, state, batch, starts, states, n_steps, num_envs, first,
                                count, cases.hyper_of(update))
        for what, x, y in zip(("params", "state", "stats", "gradient"), got, want[update]):
            assert bits(x) == bits(y), f"{name}, update {update}: {what} differ"
        params, state = got[0], got[1]
    assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()
    assert all(stats[7] == 0 for _, _, stats, _ in want) and bits(want[-1][0]) != bits(want[0][0])
    assert np.isnan(states[:, 1]).all()  # (the vf half of lstm_states is NaN throughout here, too)


# ---- 2: the packing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", cases.HEADS)
def test_packing_of_an_odd_width_network(head, hostcheck):
    """Element by element; the state_dict's names and torch shapes round-trip; a dict of the other mode is refused by name;
    P' = P - [4H(D + H) + 8H] + [DH + H]."""
    network = cases.NETWORKS[cases.ODD]
    width, hidden = network[0], network[1]
    spec, other = cases.spec_of(head, network), cases.spec_of(head, network, enable_critic_lstm=True)
    assert not spec.enable_critic_lstm and other.enable_critic_lstm and cases.spec_of(head, network, True).size == other.size
    assert spec.size == other.size - (4 * hidden * (width + hidden) + 8 * hidden) + (width * hidden + hidden)
    assert spec.critic_desc() == other.desc() + (1,) and other.critic_desc() == other.desc() + (0,)
    names = spec.keys()
    swapped = [name for name in other.keys() if not name.startswith("lstm_critic.")]
    assert [name for name in names if not name.startswith("critic.")] == swapped
    at = names.index("critic.weight")
    assert names[at + 1] == "critic.bias" and names[at - 1] == "action_net.bias"
    assert names[at + 2] == "mlp_extractor.value_net.0.weight" and (names[-1] == "log_std") == (head == "sde")
    state = cases.state_dict(head, spec, 11)
    assert state["critic.weight"].shape == (hidden, width) and state["critic.bias"].shape == (hidden,)
    params = spec.pack(state)
    bias_at = ctypes.c_ulonglong()
    sde = int(head == "sde")
    weight_at = hostcheck.lcc_critic_at(ctypes.byref(cases.critic_desc(spec)), sde, ctypes.byref(bias_at))
    entries = {name: (offset, shape) for name, offset, shape, _ in spec.entries}
    assert entries["critic.weight"] == (weight_at, (width, hidden)) and entries["critic.bias"] == (bias_at.value, (hidden,))
    assert weight_at == entries["action_net.bias"][0] + spec.n_actions  # (right after the pi net)
    assert entries["mlp_extractor.value_net.0.weight"][0] == bias_at.value + hidden
    for j in range(hidden):
        assert params[bias_at.value + j] == state["critic.bias"][j]
        for k in range(width):
            assert params[weight_at + k * hidden + j] == state["critic.weight"][j, k]
    if head == "sde":
        assert spec.log_std_at == spec.size - spec.latent and bits(params[spec.log_std_at:]) == bits(state["log_std"][:, 0])
    at = 0
    for name, offset, shape, is_weight in spec.entries:  # (every entry follows the one before: nothing else is packed)
        assert offset == at
        at += int(np.prod(shape))
    assert at == spec.size == hostcheck.lcc_params_size(ctypes.byref(cases.critic_desc(spec)), sde)
    assert other.size == hostcheck.lcc_params_size(ctypes.byref(cases.critic_desc(other)), sde)
    assert hostcheck.lcc_params_size(ctypes.byref(cases.critic_desc(spec, critic=2)), sde) == 0
    assert hostcheck.lcc_params_size(ctypes.byref(cases.critic_desc(spec, critic=-1)), sde) == 0
    back = spec.unpack(params)
    assert list(back) == names
    for name in names:
        assert back[name].shape == state[name].shape and bits(back[name]) == bits(state[name]), name
    with pytest.raises(KeyError, match="lstm_critic.weight_ih_l0.*enable_critic_lstm=True"):
        spec.pack(cases.state_dict(head, other, 11))
    with pytest.raises(KeyError, match="critic.weight.*enable_critic_lstm=False"):
        other.pack(state)
    nets = spec.nets(params)
    assert len(nets[0][0]) == 4 and len(nets[1][0]) == 2 and nets[1][0][0].shape == (width, hidden)
    assert len(nets[1][1]) == len(network[3]) and nets[1][2][0].shape == (network[3][-1], 1)


# ---- 3: what the value path and the update never read -----------------------------------------------------------------------
@pytest.mark.parametrize("head", cases.HEADS)
def test_value_path_ignores_state_and_starts(head, hostcheck):
    """With the state all NaN and every start byte 0, values and final_values are finite and byte-equal to those with a
    zero state and every start byte 1; the stored state's two halves are byte-equal."""
    n = cases.SIZES[2]
    spec, params, obs, _, _, _ = cases.chain_inputs(head, cases.ODD, n)
    finite = np.nan_to_num(obs, nan=0.25, posinf=3.0, neginf=-3.0)
    _, theta = cases.chain_noise(head, cases.ODD, n, "sampled")
    seen = []
    for fill, byte in ((np.nan, 0), (0.0, 1)):
        state = np.full(spec.state_shape(n), fill, dtype=F32)
        starts = np.full(n, byte, dtype=np.uint8)
        for forward in (lambda *a, **k: cases.twin_forward(head, *a, **k), lambda *a, **k: cases.host_forward(hostcheck, head, *a, **k)):
            full = forward(spec, params, finite[0], starts, state, finite[1], None, theta, True)
            only = forward(spec, params, finite[0], starts, state, finite[1], None, None, True, values_only=True)
            for key in ("values", "final_values"):
                assert np.isfinite(full[key]).all() and bits(full[key]) == bits(only[key]), key
            assert bits(full["state"][0]) == bits(full["state"][1]) and only["state"] is None
            seen.append((bits(full["values"]), bits(full["final_values"])))
    assert len(set(seen)) == 1
    assert np.isnan(cases.twin_forward(head, spec, params, finite[0], np.zeros(n, np.uint8), np.full(spec.state_shape(n), np.nan, F32),
                                       None, None, theta, True)["state"]).all()  # (the pi net does read its half)


@pytest.mark.parametrize("head", cases.HEADS)
def test_update_never_reads_the_vf_half(head, hostcheck):
    """The vf half of lstm_states NaN throughout against normal values there: parameters, optimizer state, stats and
    gradient are byte-equal -- and finite, and the pi half does matter."""
    name = "mixed/7/15"
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(head, cases.ODD, name)
    assert np.isnan(states[:, 1]).all()
    filled = states.copy()
    filled[:, 1] = filled[:, 0] * F32(3.0) + F32(1.0)
    state = cases.twin_updates(head, cases.ODD, name)[0][1]
    args = (n_steps, num_envs, first, count, cases.hyper_of(1))
    want = cases.twin_updates(head, cases.ODD, name)[1]
    for update in (cases.twin_update, lambda *a: cases.host_update(hostcheck, head, *a)):
        got = update(spec, cases.twin_updates(head, cases.ODD, name)[0][0], state, batch, starts, filled, *args)
        for what, x, y in zip(("params", "state", "stats", "gradient"), got, want):
            assert bits(x) == bits(y) and np.isfinite(x).all(), what
    moved = filled.copy()
    moved[:, 0] += F32(0.25)
    other = cases.twin_update(spec, cases.twin_updates(head, cases.ODD, name)[0][0], state, batch, starts, moved, *args)
    assert bits(other[3]) != bits(want[3])
    no_starts = np.ones_like(starts)  # (episode_starts reaches the value path nowhere: the critic's gradient stays)
    other = cases.twin_update(spec, cases.twin_updates(head, cases.ODD, name)[0][0], state, batch, no_starts, filled, *args)
    entries = {entry[0]: entry for entry in spec.entries}
    first_vf, last_vf = entries["critic.weight"][1], entries["value_net.bias"][1] + 1
    assert bits(other[3][first_vf:last_vf]) == bits(want[3][first_vf:last_vf]) and np.abs(want[3][first_vf:last_vf]).max() > 0
    assert bits(other[3][:first_vf]) != bits(want[3][:first_vf])


# ---- 4: the meaning, against torch in float64 -------------------------------------------------------------------------------------
AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST = 8, 4, 5


def autograd_inputs(head, index):
    """The sibling test's inputs (tests/test_lstm_learner_logic.py): a rollout of 8 steps of 4 environments taken as ONE
    minibatch of 32 rows rotated by 5; environment 1 runs all 8 rows from a stored non-zero state, the others start
    episodes inside.  The stored log-probabilities are the twin's own plus normal noise of scale 0.15."""
    from reinfocus_amd.environments import sde

    spec = cases.spec_of(head, cases.NETWORKS[index])
    state = cases.state_dict(head, spec, 60 + index)
    params = spec.pack(state)
    n_steps, num_envs = AUTOGRAD_STEPS, AUTOGRAD_ENVS
    total = n_steps * num_envs
    rng = np.random.default_rng(index)
    starts = np.zeros((n_steps + 1, num_envs), dtype=np.uint8)
    starts[0, 0], starts[3, 0], starts[5, 2], starts[0, 3], starts[6, 3] = 1, 1, 1, 1, 1
    states = cases.nan_vf_half(0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs)))
    batch = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32)}
    if head == "categorical":
        batch["actions"] = rng.integers(0, spec.n_actions, total).astype(np.int64)
    batch["advantages"], batch["returns"] = rng.standard_normal(total).astype(F32), rng.standard_normal(total).astype(F32)
    if head == "sde":
        mu, sigma, h = lstm_sde_cases.own_head(spec, params, batch, starts, states, n_steps, num_envs)
        theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(total * spec.latent))
        with np.errstate(all="ignore"):
            batch["actions"] = policy.canonical(mu + sde._rowdot(h, theta))
        own = sde.log_prob_of(batch["actions"], mu, sigma)
    else:
        own = cases.lstm_learner_cases.own_log_probs(spec, params, batch, starts, states, n_steps, num_envs)
    batch["log_probs"] = (own + 0.15 * rng.standard_normal(total)).astype(F32)
    return spec, state, params, batch, starts, states


def twin_heads(spec, params, batch, starts, states, rows):
    """The twins' forward on the minibatch's rows: (logits [B, A] or the mean [B, 1], values [B])."""
    index = np.array([row[0] for row in rows])
    x = batch["observations"][index]
    (pi_lstm, pi_layers, pi_last), (critic, vf_layers, vf_last) = spec.nets(params)
    with np.errstate(all="ignore"):
        h = lstm_learner._cell_rows(x, rows, (states[:, 0, 0], states[:, 0, 1]), pi_lstm)[4]
        v = policy.linear(x, *critic)
        for weight_t, bias in pi_layers:
            h = policy.activation(policy.linear(h, weight_t, bias), spec.activation)
        for weight_t, bias in vf_layers:
            v = policy.activation(policy.linear(v, weight_t, bias), spec.activation)
        return policy.linear(h, *pi_last), policy.linear(v, *vf_last)[:, 0]


@pytest.mark.parametrize("index", [cases.TUNED, cases.ODD], ids=[NETWORK_IDS[cases.TUNED], NETWORK_IDS[cases.ODD]])
@pytest.mark.parametrize("head", cases.HEADS)
def test_forward_gradient_and_updates_are_no_further_from_float64_than_four_times_torch(head, index, tmp_path, hostcheck):
    """The twin's logits (the mean with the Gaussian head) and values on the minibatch, its gradient before clipping, its
    parameters after the first update of a fresh optimizer and after 10 updates, each against the same from torch in
    float64 (torch.nn.LSTM cells stepped per row for the actor with the definition's sequence rule and select,
    torch.nn.Linear for `critic` on the observations alone, stable-baselines3's loss, autograd, clip_grad_norm_,
    Adam(eps=1e-5)): the largest distance may be at most 4 x that of torch's own float32 run on the same inputs -- the
    allowance of the sibling tests.  And the critic layer is really trained: with the layer left out of the graph, torch's
    float64 gradient of critic.weight moves by far more than that bound.  Every distance is printed."""
    spec, state, params, batch, starts, states = autograd_inputs(head, index)
    n_steps, num_envs, first, count = AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST, AUTOGRAD_STEPS * AUTOGRAD_ENVS
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    hyper = learner.Hyper(3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1)
    updates = 10
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), activation=spec.activation, obs=batch["observations"],
             actions=batch["actions"], old_log_probs=batch["log_probs"], advantages=batch["advantages"],
             returns=batch["returns"], lstm_states=np.nan_to_num(states, nan=0.0),
             row=np.array([row[0] for row in rows], dtype=np.int64), env=np.array([row[1] for row in rows], dtype=np.int64),
             step=np.array([row[2] for row in rows], dtype=np.int64), is_start=np.array([row[3] for row in rows]),
             zero=np.array([row[4] for row in rows]), clip_range=hyper.clip_range, ent_coef=hyper.ent_coef,
             vf_coef=hyper.vf_coef, max_grad_norm=hyper.max_grad_norm, learning_rate=hyper.learning_rate, updates=updates,
             **state)
    subprocess.run([sys.executable, "-m", "tests.lstm_critic_io_cases", "--torch-critic-learner", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=600)
    theirs = np.load(tmp_path / "out.npz")
    grad, terms, invalid = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first,
                                                            count, hyper)
    assert not invalid and np.isfinite(grad).all()
    head_out, values = twin_heads(spec, params, batch, starts, states, rows)
    ours = {"head": head_out, "values": values, "grad": grad}
    optimizer = learner.fresh_state(spec)
    for update in range(updates):
        params, optimizer, stats = lstm_learner.lstm_update_numpy(spec, params, optimizer, batch, starts, states, n_steps,
                                                                  num_envs, first, count, hyper)
        assert stats[7] == 0
        if update == 0:
            ours["first"] = params
    ours["last"] = params
    assert bits(cases.host_update(hostcheck, head, spec, spec.pack(state), learner.fresh_state(spec), batch, starts, states,
                                  n_steps, num_envs, first, count, hyper)[3]) == bits(grad)
    bound = None
    label = f"{head} {cases.NETWORKS[index]}"
    for kind in ("head", "values", "grad", "first", "last"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64 and exact.shape == ours[kind].shape
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{label}: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        assert twin <= 4.0 * torch, (kind, twin, torch)
        if kind == "grad":
            bound = 4.0 * torch
    for name, at, shape, _ in spec.entries:
        if name.startswith("critic."):
            size = int(np.prod(shape))
            moved = np.abs(theirs["grad_without64"][at:at + size] - theirs["grad64"][at:at + size]).max()
            print(f"{label}: {name}: leaving the layer out moves the float64 gradient by {moved:.3e}, the bound is {bound:.3e}")
            assert moved > 1000.0 * bound, (name, moved, bound)


# ---- 5: the binding ------------------------------------------------------------------------------------------------------------------
SIBLINGS = {"rf_lstm_critic_params_size": "rf_lstm_params_size", "rf_lstm_critic_forward": "rf_lstm_forward",
            "rf_lstm_critic_ppo_state_size": "rf_lstm_ppo_state_size",
            "rf_lstm_critic_ppo_workspace_size": "rf_lstm_ppo_workspace_size",
            "rf_lstm_critic_ppo_update": "rf_lstm_ppo_update", "rf_lstm_critic_sde_params_size": "rf_lstm_sde_params_size",
            "rf_lstm_critic_sde_noise_reset": "rf_lstm_sde_noise_reset", "rf_lstm_critic_sde_forward": "rf_lstm_sde_forward",
            "rf_lstm_critic_sde_state_size": "rf_lstm_sde_state_size",
            "rf_lstm_critic_sde_workspace_size": "rf_lstm_sde_workspace_size",
            "rf_lstm_critic_sde_update": "rf_lstm_sde_update"}


def test_binding_matches_the_header():
    """The new struct and every new entry point: the header's declaration, the binding's argtypes and restype, the
    definition in the library's source; each sibling takes its rf_lstm_ function's arguments over rf_lstm_critic_desc.  The
    existing struct is untouched."""
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef struct rf_lstm_critic_desc \{\s*rf_lstm_policy_desc lstm;\s*int critic;\s*\} rf_lstm_critic_desc;",
                     text)
    assert re.search(r"#define RF_LSTM_CRITIC_LSTM 0\n#define RF_LSTM_CRITIC_LINEAR 1\n", text)
    assert (_native.LSTM_CRITIC_LSTM, _native.LSTM_CRITIC_LINEAR) == (lstm.CRITIC_LSTM, lstm.CRITIC_LINEAR) == (0, 1)
    assert [name for name, _ in _native.LstmCriticDesc._fields_] == ["lstm", "critic"]
    assert _native.LstmCriticDesc._fields_[0][1] is _native.LstmPolicyDesc and _native.LstmCriticDesc._fields_[1][1] is ctypes.c_int
    assert ctypes.sizeof(_native.LstmCriticDesc) == ctypes.sizeof(_native.LstmPolicyDesc) + 4 == 44
    assert [name for name, _ in _native.LstmPolicyDesc._fields_] == ["policy", "lstm_hidden"]
    assert re.search(r"typedef struct rf_lstm_policy_desc \{\s*rf_policy_desc policy;\s*int lstm_hidden;\s*\} rf_lstm_policy_desc;",
                     text)
    desc = _native.LstmCriticDesc(*range(1, 12))
    assert (desc.lstm.policy.obs_width, desc.lstm.policy.vf_width[1], desc.lstm.lstm_hidden, desc.critic) == (1, 9, 10, 11)
    lib = _native.load()
    abi = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_abi_env.hip")).read()
    for entry, sibling in SIBLINGS.items():
        ours = re.search(r"\b%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1)
        theirs = re.search(r"\b%s\s*\((.*?)\)\s*;" % sibling, text, flags=re.S).group(1)
        squeeze = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
        assert squeeze(ours) == squeeze(theirs).replace("rf_lstm_policy_desc", "rf_lstm_critic_desc"), entry
        wanted = [ctypes.c_void_p if "*" in p or "[" in p else ctypes.c_int for p in ours.split(",")]
        assert getattr(lib, entry).argtypes == wanted == getattr(lib, sibling).argtypes, entry
        size = entry.endswith("_size")
        assert getattr(lib, entry).restype is (ctypes.c_ulonglong if size else ctypes.c_int), entry
        assert entry in _native.SYMBOLS
        assert re.search(r"\n(int|unsigned long long) %s\(rf_ctx \*ctx, const rf_lstm_critic_desc \*desc" % entry, abi), entry
    for kept in ("rf_lstm_forward", "rf_lstm_ppo_update", "rf_lstm_sde_forward", "rf_lstm_sde_update", "rf_lstm_state_size"):
        assert re.search(r"\n(int|unsigned long long) %s\(rf_ctx \*ctx, const rf_lstm_policy_desc \*desc" % kept, abi), kept


@pytest.mark.parametrize("head", cases.HEADS)
def test_workspace_is_smaller_than_the_lstm_critics(head, hostcheck):
    """At equal batch, for every network and several batches; the difference is the vf net's h_prev, c_prev, gates, c' and
    da (11 H floats per row) less the shorter gradient and its partial sums."""
    sde = int(head == "sde")
    for network in cases.NETWORKS:
        spec = cases.spec_of(head, network)
        for batch in (1, 8, 9, 128, 1024):
            ours = hostcheck.lcc_workspace_size(ctypes.byref(cases.critic_desc(spec)), sde, batch)
            theirs = hostcheck.lcc_workspace_size(ctypes.byref(cases.critic_desc(spec, critic=0)), sde, batch)
            assert 0 < ours < theirs and ours % 8 == 0, (network, batch, ours, theirs)
            assert theirs - ours >= 4 * 11 * spec.lstm_hidden * batch
            if head == "sde":
                lstm_lib = lstm_sde_cases.hostcheck()
                assert theirs == lstm_lib.lsc_workspace_size(ctypes.byref(_native.LstmPolicyDesc(*spec.desc())), batch)
        assert hostcheck.lcc_workspace_size(ctypes.byref(cases.critic_desc(spec)), sde, 0) == 0
        assert hostcheck.lcc_workspace_size(ctypes.byref(cases.critic_desc(spec)), sde, 1025) == 0
        assert hostcheck.lcc_workspace_size(ctypes.byref(cases.critic_desc(spec, critic=2)), sde, 8) == 0


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd import _native; from reinfocus_amd.environments import harness, lstm, lstm_sde; "
            "_native.LstmCriticDesc; _native.Context.lstm_critic_forward; _native.Context.lstm_critic_ppo_update; "
            "lstm.LstmPolicySpec(4, 3, enable_critic_lstm=False).critic_desc(); "
            "lstm_sde.LstmSdePolicySpec(4, enable_critic_lstm=False); lstm.vf_latents; "
            "harness.LstmPolicy(lstm.LstmPolicySpec(4, 3, lstm_hidden=8, enable_critic_lstm=False), 0, num_envs=2); "
            "assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_twin_classes_work_from_the_spec():
    """LstmPolicy / LstmSdePolicy / LstmLearner over a spec of this mode: act() stores equal halves, values() ignores the
    state, an update moves critic.weight; state_dict() / load_state_dict() round-trip under the new names."""
    from reinfocus_amd.environments import harness

    for head in cases.HEADS:
        spec = cases.spec_of(head, cases.NETWORKS[cases.TUNED])
        n = 3
        twin = (harness.LstmSdePolicy if head == "sde" else harness.LstmPolicy)(spec, 5, num_envs=n)
        twin.load_state_dict(cases.state_dict(head, spec, 3))
        assert "critic.weight" in twin.state_dict() and "lstm_critic.weight_ih_l0" not in twin.state_dict()
        obs = np.random.default_rng(1).standard_normal((n, spec.obs_width)).astype(F32)
        if head == "sde":
            twin.reset_noise(n)
        twin.act(obs, np.ones(n, np.uint8))
        state = twin.lstm_state()
        assert bits(state[0]) == bits(state[1]) and np.abs(state).max() > 0
        before = twin.values(obs, np.zeros(n, np.uint8))
        twin.set_lstm_state(np.full_like(state, np.nan))
        assert bits(twin.values(obs, np.zeros(n, np.uint8))) == bits(before) and np.isfinite(before).all()
        assert isinstance(harness.LstmLearner(twin), lstm_learner.LstmLearner)
    for refused in (dict(lstm_hidden=512), dict(lstm_hidden=257)):  # (still out of scope)
        with pytest.raises(ValueError):
            lstm.LstmPolicySpec(4, 3, enable_critic_lstm=False, **refused)
        with pytest.raises(ValueError):
            lstm_sde.LstmSdePolicySpec(4, enable_critic_lstm=False, **refused)
    assert lstm_cases.spec_of(cases.NETWORKS[cases.TUNED]).enable_critic_lstm  # (the default is the LSTM critic)
