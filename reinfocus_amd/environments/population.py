"""A population of G independent PPO learners in lock-step over ONE vector environment of n = G m lanes: seed sweeps, the
reference's side-by-side hyper-parameter trials (where they share an architecture), population-based training.  The
reference trains with n_envs 8; at 8 environments a forward is one or two blocks and an update three launch-bound kernels,
so G separate policy / learner objects cost G (1 + 3 updates) launches per iteration on an idle device.  Here every stage
of all G learners is one launch.

One definition (include/reinfocus_hip.h, "population"): the arithmetic of a group is exactly that of "policy" and "ppo
update"; only addressing changes.  Group g owns environments [g m, (g + 1) m), parameters params[g], its own generator,
optimizer state, hyper-parameters and stats, and rows [g m T, (g + 1) m T) of a rollout's flat() (which orders rows
e T + t, so the rows of consecutive environments are contiguous).

    PopulationPolicy         the numpy twin: literally G policy.Policy over slices, and the oracle
    PopulationLearner        the numpy twin: literally G learner.Learner over slices
    DevicePopulationPolicy   act / values over all n rows in ONE launch (rf_policy_forward_grouped); spec.kind is the mlp
                             kind, so Rollout.collect / DeviceRollout.collect take it as they take a Policy / DevicePolicy
    DevicePopulationLearner  update / train: three launches per minibatch whatever G is (rf_ppo_update_grouped)

The Gaussian head (include/reinfocus_hip.h, "population sde"): G gSDE learners over a Box(-1, 1, (1,)) action space, each
group with its own log_std (log_std_init per group) and its own noise schedule (collect(sde_sample_freq=G values)), as
the reference's search draws both per trial for ContinuousJumps-v0.

    SdePopulationPolicy        the numpy twin: literally G sde.SdePolicy over slices, and the oracle
    DeviceSdePopulationPolicy  reset_noise(groups=mask) / act / values in ONE launch each (rf_sde_noise_reset_grouped,
                               rf_sde_forward_grouped); spec.kind is the sde kind
    PopulationLearner / DevicePopulationLearner take them as they take the Categorical ones and dispatch on the spec's
    kind (G learner.Learner over SdePolicy members; rf_sde_update_grouped)

A normaliser and GAE discounts per group (include/reinfocus_hip.h, "population view"): an environment built with
learner_view=harness.LearnerView(..., gamma=scalar | G values, groups=G) keeps running moments per group, taken over the
group's own lanes, and rollout.Rollout / DeviceRollout(env, n_steps, gamma, gae_lambda, groups=G) take a gamma and a
gae_lambda per group -- what a stand-alone trial over m environments normalises and discounts by.  VecNormalize's gamma
(the view's) and the rollout's gamma are passed separately; rl_zoo3 sets both from the trial's gamma.

The recurrent head (include/reinfocus_hip.h, "population lstm"): G recurrent PPO learners (the Categorical head on the
LSTM, either critic kind), as the reference's search runs its ppo_lstm sampler.

    LstmPopulationPolicy         the numpy twin: literally G lstm.LstmPolicy over lane slices, and the oracle
    DevicePopulationLstmPolicy   act / values in ONE launch (rf_lstm_forward_grouped); the state keeps its single form
                                 [2][2][n][H], so rollout slabs, lstm_state(), snapshots and collect() do not change shape;
                                 spec.kind is the lstm kind, so collect() keeps episode_starts and lstm_states
    PopulationLearner / DevicePopulationLearner become the recurrent learner with them: update(rollout_or_parts, firsts,
    count) and train(rollout, n_epochs, batch_size, splits) as lstm_learner's, with one first row / split per group
    (G lstm_learner.LstmLearner over slice-parts; rf_lstm_ppo_update_grouped, six launches whatever G is)

The recurrent Gaussian head (include/reinfocus_hip.h, "population lstm sde"): G recurrent gSDE learners over a
Box(-1, 1, (1,)) action space -- both rules at once, as the reference's ppo_lstm search runs ContinuousJumps-v0: each group
with its own log_std_init and sde_sample_freq, the state in its single form, float32 raw actions in the update.

    LstmSdePopulationPolicy        the numpy twin: literally G lstm_sde.LstmSdePolicy over lane slices, and the oracle
    DevicePopulationLstmSdePolicy  reset_noise(groups=mask) / act / values in ONE launch each
                                   (rf_lstm_sde_noise_reset_grouped, rf_lstm_sde_forward_grouped); spec.kind is the
                                   lstm_sde kind, so collect() keeps episode_starts and lstm_states and resets the noise
                                   per group
    PopulationLearner / DevicePopulationLearner become the recurrent learner over float32 raw actions with them
    (G lstm_learner.LstmLearner over LstmSdePolicy members; rf_lstm_sde_update_grouped, six launches whatever G is)

Out of scope: groups that differ in architecture, critic kind, m, T or batch size; more than one action
dimension; SB3Wrapper; and the environment's shared reset-state generator -- lanes that end are
ranked across all groups, so which reset state a lane draws depends on other groups' episode ends: the independence
covers what the learner is given the raw step, not the environment's draws.

torch is imported lazily, by the device classes only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import numpy as np

from reinfocus_amd.environments import learner as learner_module
from reinfocus_amd.environments import lstm as lstm_module
from reinfocus_amd.environments import lstm_learner as lstm_learner_module
from reinfocus_amd.environments import lstm_sde as lstm_sde_module
from reinfocus_amd.environments import policy as policy_module
from reinfocus_amd.environments import sde as sde_module
from reinfocus_amd.environments.learner import MAX_BATCH, STATE_HEADER, f64
from reinfocus_amd.environments.policy import DETERMINISTIC, f32

MAX_GROUPS = 65535  # RF_POPULATION_MAX_GROUPS
# rf_ppo_hyper: what one group's kernels read of its hyper-parameters (56 bytes)
HYPER_RECORD = np.dtype([("learning_rate", f64), ("max_grad_norm", f64), ("beta1", f64), ("beta2", f64), ("adam_eps", f64),
                         ("clip_range", f32), ("ent_coef", f32), ("vf_coef", f32), ("normalize_advantage", np.int32)])
assert HYPER_RECORD.itemsize == 56


def _checked_population(spec, groups, seeds):
    if getattr(spec, "kind", None) != policy_module.MlpPolicySpec.kind:
        raise ValueError(f"a population has the Categorical head of MlpPolicySpec, not a spec of kind "
                         f"{getattr(spec, 'kind', None)!r}: the sde and lstm heads are out of scope")
    return _checked_groups(groups, seeds)


def _checked_groups(groups, seeds):
    groups = int(groups)
    if not 1 <= groups <= MAX_GROUPS:
        raise ValueError(f"groups {groups} is not in 1 .. {MAX_GROUPS}")
    seeds = list(seeds) if isinstance(seeds, (list, tuple, np.ndarray)) else None
    if seeds is None or len(seeds) != groups:
        raise ValueError(f"seeds must be a sequence of one seed per group ({groups}), not "
                         f"{'a scalar' if seeds is None else len(seeds)}")
    return groups, seeds


def _checked_sde_population(spec, groups, seeds, log_std_init):
    """(G, seeds, log_std_init per group) of a population with the Gaussian head."""
    if getattr(spec, "kind", None) != sde_module.SdePolicySpec.kind:
        raise ValueError(f"a population of gSDE learners has the Gaussian head of SdePolicySpec, not a spec of kind "
                         f"{getattr(spec, 'kind', None)!r}: MlpPolicySpec has PopulationPolicy / DevicePopulationPolicy, "
                         "the lstm heads are out of scope")
    groups, seeds = _checked_groups(groups, seeds)
    inits = per_group(spec.log_std_init if log_std_init is None else log_std_init, groups, "log_std_init")
    return groups, seeds, np.array([float(x) for x in inits], dtype=f32)


LSTM_KIND = "lstm"  # (LstmPolicySpec.kind)


def _checked_lstm_population(spec, groups, seeds):
    if getattr(spec, "kind", None) != LSTM_KIND:
        raise ValueError(f"a population of recurrent learners has the Categorical head of LstmPolicySpec, not a spec of kind "
                         f"{getattr(spec, 'kind', None)!r}: MlpPolicySpec has PopulationPolicy / DevicePopulationPolicy, "
                         "SdePolicySpec SdePopulationPolicy / DeviceSdePopulationPolicy; the lstm-sde head (LstmSdePolicySpec) "
                         "in a population is out of scope here -- it is the next step, LstmSdePopulationPolicy / "
                         "DevicePopulationLstmSdePolicy")
    return _checked_groups(groups, seeds)


LSTM_SDE_KIND = lstm_sde_module.LstmSdePolicySpec.kind
RECURRENT_KINDS = (LSTM_KIND, LSTM_SDE_KIND)


def _checked_lstm_sde_population(spec, groups, seeds, log_std_init):
    """(G, seeds, log_std_init per group) of a population with the Gaussian head on the LSTM."""
    if getattr(spec, "kind", None) != LSTM_SDE_KIND:
        raise ValueError(f"a population of recurrent gSDE learners has the Gaussian head of LstmSdePolicySpec, not a spec of "
                         f"kind {getattr(spec, 'kind', None)!r}: MlpPolicySpec has PopulationPolicy / DevicePopulationPolicy, "
                         "SdePolicySpec SdePopulationPolicy / DeviceSdePopulationPolicy, LstmPolicySpec LstmPopulationPolicy / "
                         "DevicePopulationLstmPolicy")
    groups, seeds = _checked_groups(groups, seeds)
    inits = per_group(spec.log_std_init if log_std_init is None else log_std_init, groups, "log_std_init")
    return groups, seeds, np.array([float(x) for x in inits], dtype=f32)


def group_parts(parts, groups, g):
    """Group g's slice of parts_of(rollout) over n = G m lanes, as a stand-alone rollout of m lanes would hand it over:
    rows [g m T, (g + 1) m T) of the flat arrays, columns [g m, (g + 1) m) of episode_starts and lstm_states (views)."""
    steps, lanes = int(parts["n_steps"]), int(parts["num_envs"])
    m = _per_group(lanes, groups)
    rows = m * steps
    out = {key: parts[key][g * rows:(g + 1) * rows] for key in learner_module.BATCH_KEYS}
    out.update(episode_starts=parts["episode_starts"][:, g * m:(g + 1) * m],
               lstm_states=parts["lstm_states"][:, :, :, g * m:(g + 1) * m, :], n_steps=steps, num_envs=m)
    return out


def _checked_firsts(firsts, groups, rows, what="firsts"):
    """G integers in 0 .. rows - 1."""
    values = np.asarray(firsts)
    if values.shape != (groups,) or not np.issubdtype(values.dtype, np.integer) or values.min() < 0 or values.max() >= rows:
        raise ValueError(f"{what} must be {groups} integers in 0 .. {rows - 1}, one per group, not {firsts!r}")
    return [int(v) for v in values]


def _group_splits(splits, n_epochs, groups, rows, generator):
    """The split index of every epoch and group, int [n_epochs][G]: `splits` if given, else generator.integers(rows,
    size=G) per epoch (a host draw)."""
    if splits is not None:
        values = np.asarray(splits)
        if values.shape != (n_epochs, groups) or not np.issubdtype(values.dtype, np.integer) or values.min() < 0 \
                or values.max() >= rows:
            raise ValueError(f"splits must be integers in 0 .. {rows - 1} of shape ({n_epochs}, {groups}): one per epoch and "
                             f"group, not shape {values.shape}")
        return values.astype(np.int64)
    if generator is None:
        generator = np.random.default_rng()
    return np.stack([generator.integers(rows, size=groups) for _ in range(n_epochs)]).astype(np.int64)


def _refuse_other_groups(rollout, groups):
    other = getattr(rollout, "groups", None)
    if other is not None and int(other) != groups:
        raise ValueError(f"the rollout was made with groups={other}, the population has {groups} groups")


def _initial_params(spec, inits):
    """float32 [G][P + L]: spec.initial() per group, with the group's own log_std_init."""
    params = np.tile(spec.initial(), (len(inits), 1))
    params[:, spec.log_std_at:] = inits[:, None]
    return params


def group_mask(selected, groups):
    """`selected` as a bool array [G]: None for every group, else a boolean sequence of length G."""
    if selected is None:
        return np.ones(groups, dtype=bool)
    mask = np.asarray(selected)
    if mask.shape != (groups,) or mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)) or mask.max(initial=0) > 1:
        raise ValueError(f"groups must be None or a boolean sequence of one entry per group ({groups}), not {selected!r}")
    return mask.astype(bool)


def _per_group(lanes, groups):
    """m of n = G m; ValueError where the groups do not divide the lanes."""
    if lanes < groups or lanes % groups != 0:
        raise ValueError(f"{lanes} environments are not divisible into {groups} groups of at least one")
    return lanes // groups


def per_group(value, groups, name):
    """`value` as a list of one entry per group: a scalar for all, or a sequence of length G."""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != groups:
            raise ValueError(f"{name} has {len(value)} entries, the population {groups} groups")
        return list(value)
    return [value] * groups


def _betas_per_group(betas, groups):
    betas = list(betas)
    if len(betas) == 2 and not any(isinstance(b, (list, tuple, np.ndarray)) for b in betas):
        return [tuple(betas)] * groups
    if len(betas) != groups or not all(len(b) == 2 for b in betas):
        raise ValueError(f"betas is a pair, or one pair per group ({groups})")
    return [tuple(b) for b in betas]


class _GroupHyper:
    """The hyper-parameters as plain attributes, each a scalar (for every group) or a sequence of one value per group;
    they may be changed between calls."""

    def _configure(self, learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps):
        self.learning_rate, self.clip_range, self.ent_coef, self.vf_coef = learning_rate, clip_range, ent_coef, vf_coef
        self.max_grad_norm, self.normalize_advantage, self.betas, self.adam_eps = (max_grad_norm, normalize_advantage,
                                                                                   betas, adam_eps)
        self.hypers()

    def hypers(self):
        """One learner.Hyper per group; ValueError for what rf_ppo_update refuses or a sequence of the wrong length."""
        groups = self.groups
        columns = [per_group(getattr(self, name), groups, name)
                   for name in ("learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm")]
        betas = _betas_per_group(self.betas, groups)
        eps = per_group(self.adam_eps, groups, "adam_eps")
        normalize = per_group(self.normalize_advantage, groups, "normalize_advantage")
        return [learner_module.checked_hyper((*(column[g] for column in columns), betas[g][0], betas[g][1], eps[g],
                                              normalize[g])) for g in range(groups)]

    def _batches(self, rows, n_epochs, batch_size):
        n_epochs, batch_size = int(n_epochs), int(batch_size)
        if n_epochs < 1 or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError(f"n_epochs {n_epochs} must be at least 1 and batch_size {batch_size} in 1 .. {MAX_BATCH}")
        if batch_size > rows:
            raise ValueError(f"batch_size {batch_size} is more than the {rows} rows (m T) of one group")
        return n_epochs, batch_size, -(-rows // batch_size)


def hyper_records(hypers):
    """The G rf_ppo_hyper records of a list of learner.Hyper, as the kernels read them."""
    records = np.zeros(len(hypers), dtype=HYPER_RECORD)
    for g, hyper in enumerate(hypers):
        records[g] = (hyper.learning_rate, hyper.max_grad_norm, hyper.beta1, hyper.beta2, hyper.adam_eps,
                      f32(hyper.clip_range), f32(hyper.ent_coef), f32(hyper.vf_coef), hyper.normalize_advantage)
    return records


def _refuse_rollout(spec, rollout):
    """A Categorical population refuses a Box rollout, one with the Gaussian head a Discrete one."""
    if spec.kind == sde_module.SdePolicySpec.kind:
        sde_module._refuse_discrete(rollout.env.single_action_space)
    elif spec.kind == LSTM_SDE_KIND:
        lstm_sde_module._refuse_discrete(rollout.env.single_action_space)
    elif spec.kind == LSTM_KIND:
        lstm_module._refuse_box(rollout.env.single_action_space)
    else:
        policy_module._refuse_box(rollout.env.single_action_space)


class PopulationPolicy:
    """The numpy twin of DevicePopulationPolicy, and its oracle: G policy.Policy, group g seeded with seeds[g], over
    slices of the rows.  `params` is one array [G][P]; policies[g].params is its row g."""

    def __init__(self, spec, groups, seeds):
        self.groups, seeds = _checked_population(spec, groups, seeds)
        self.spec = spec
        self.params = np.zeros((self.groups, spec.size), dtype=f32)
        self.policies = [policy_module.Policy(spec, seed) for seed in seeds]
        for g, member in enumerate(self.policies):
            member.params = self.params[g]

    def _groups_of(self, group):
        if group is None:
            return range(self.groups)
        if not 0 <= int(group) < self.groups:
            raise IndexError(f"group {group} is not in 0 .. {self.groups - 1}")
        return [int(group)]

    def load_state_dict(self, state_dict, group=None):
        """Into group `group`, or into every group with None."""
        packed = self.spec.pack(state_dict)
        for g in self._groups_of(group):
            self.params[g] = packed

    def state_dict(self, group=0):
        return self.spec.unpack(self.params[self._groups_of(group)[0]])

    def init_parameters(self, seeds, ortho_init=True, groups=None):
        """Policy.init_parameters per group: group g's row of `params` from seeds[g] (environments/param_init.py), with
        the group's own log_std_init where the head has one.  groups: None for every group, else G booleans -- an
        unselected group (a slot whose trial goes on) keeps its bytes.  The action generators are untouched."""
        from reinfocus_amd.environments import param_init

        param_init.init_twin(self.params, self.spec, seeds, ortho_init, groups, getattr(self, "_log_std_inits", None))

    def _split(self, obs, final_obs):
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        m = _per_group(obs.shape[0], self.groups)
        if final_obs is not None:
            final_obs = np.asarray(final_obs, dtype=f32).reshape(obs.shape)
        return [(obs[g * m:(g + 1) * m], None if final_obs is None else final_obs[g * m:(g + 1) * m])
                for g in range(self.groups)]

    def act(self, obs, final_obs=None, deterministic=False):
        """(actions int64 [n], values, log_probs, final_values or None) over all n = G m rows: group g's rows by
        policies[g], which draws m of its own generator's numbers unless deterministic."""
        parts = [member.act(rows, final_rows, deterministic)
                 for member, (rows, final_rows) in zip(self.policies, self._split(obs, final_obs))]
        return tuple(None if parts[0][i] is None else np.concatenate([part[i] for part in parts]) for i in range(4))

    def values(self, obs, final_obs=None):
        parts = [member.values(rows, final_rows)
                 for member, (rows, final_rows) in zip(self.policies, self._split(obs, final_obs))]
        if final_obs is None:
            return np.concatenate(parts)
        return np.concatenate([part[0] for part in parts]), np.concatenate([part[1] for part in parts])

    def rng_state(self):
        """The G generator states, in group order."""
        return [member.rng_state() for member in self.policies]

    def set_rng_state(self, states):
        states = list(states)
        if len(states) != self.groups:
            raise ValueError(f"{len(states)} generator states for {self.groups} groups")
        for member, state in zip(self.policies, states):
            member.set_rng_state(state)


class SdePopulationPolicy:
    """The numpy twin of DeviceSdePopulationPolicy, and its oracle: G sde.SdePolicy, group g seeded with seeds[g], over
    slices of the rows.  `params` is one array [G][P + L]; policies[g].params is its row g.  log_std_init: a scalar or G
    values, which override the spec's per group.  num_envs (n = G m; reset_noise(num_envs=) sets it) says how many rows
    of noise a group draws: m L draws of its own generator per reset."""

    def __init__(self, spec, groups, seeds, log_std_init=None):
        self.groups, seeds, inits = _checked_sde_population(spec, groups, seeds, log_std_init)
        self.spec = spec
        self.params = _initial_params(spec, inits)
        self._log_std_inits = inits
        self.policies = [sde_module.SdePolicy(spec, seed) for seed in seeds]
        for g, member in enumerate(self.policies):
            member.params = self.params[g]
        self.num_envs = self.groups

    _groups_of = PopulationPolicy._groups_of
    load_state_dict = PopulationPolicy.load_state_dict
    state_dict = PopulationPolicy.state_dict
    init_parameters = PopulationPolicy.init_parameters
    _split = PopulationPolicy._split
    values = PopulationPolicy.values
    rng_state = PopulationPolicy.rng_state
    set_rng_state = PopulationPolicy.set_rng_state

    def reset_noise(self, groups=None, num_envs=None):
        """A new theta [m, L] for every selected group (None: every group; else a boolean sequence of length G) from the
        group's current log_std: m L draws of each selected group's generator.  An unselected group keeps its theta and
        its generator state."""
        mask = group_mask(groups, self.groups)
        m = _per_group(self.num_envs if num_envs is None else int(num_envs), self.groups)
        self.num_envs = m * self.groups
        for member, selected in zip(self.policies, mask):
            if selected:
                member.reset_noise(m)

    def noise(self):
        """theta float32 [n, L] (a copy), or None while a group has none."""
        parts = [member.noise() for member in self.policies]
        return None if any(part is None for part in parts) else np.concatenate(parts)

    def set_noise(self, theta):
        if theta is None:
            for member in self.policies:
                member.set_noise(None)
            return
        theta = np.asarray(theta, dtype=f32).reshape(-1, self.spec.latent)
        m = _per_group(theta.shape[0], self.groups)
        for g, member in enumerate(self.policies):
            member.set_noise(theta[g * m:(g + 1) * m])

    def act(self, obs, final_obs=None, deterministic=False):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped)) over all
        n = G m rows: group g's rows by policies[g] and its theta.  No draw is consumed."""
        parts = [member.act(rows, final_rows, deterministic)
                 for member, (rows, final_rows) in zip(self.policies, self._split(obs, final_obs))]
        return tuple(None if parts[0][i] is None else np.concatenate([part[i] for part in parts]) for i in range(5))


class LstmPopulationPolicy:
    """The numpy twin of DevicePopulationLstmPolicy, and its oracle: G lstm.LstmPolicy, group g seeded with seeds[g], over
    slices of the lanes.  `params` is one array [G][P]; policies[g].params is its row g.  The state is ONE array
    [2, 2, n, H] over all n = G m lanes (None before the first call of a population built without num_envs); group g's
    member works on its columns [g m, (g + 1) m)."""

    def __init__(self, spec, groups, seeds, num_envs=None):
        self.groups, seeds = _checked_lstm_population(spec, groups, seeds)
        self.spec = spec
        self.params = np.zeros((self.groups, spec.size), dtype=f32)
        self.policies = [lstm_module.LstmPolicy(spec, seed) for seed in seeds]
        for g, member in enumerate(self.policies):
            member.params = self.params[g]
        self._state = None
        if num_envs is not None:
            _per_group(int(num_envs), self.groups)
            self._state = np.zeros(spec.state_shape(num_envs), dtype=f32)

    _groups_of = PopulationPolicy._groups_of
    load_state_dict = PopulationPolicy.load_state_dict
    state_dict = PopulationPolicy.state_dict
    init_parameters = PopulationPolicy.init_parameters
    rng_state = PopulationPolicy.rng_state
    set_rng_state = PopulationPolicy.set_rng_state

    def _own_state(self, n):
        if self._state is None or self._state.shape[2] != n:
            self._state = np.zeros(self.spec.state_shape(n), dtype=f32)
        return self._state

    def lstm_state(self):
        """A copy of the state float32 [2, 2, n, H] (None before the first call of a population built without num_envs)."""
        return None if self._state is None else self._state.copy()

    def set_lstm_state(self, state):
        state = np.array(state, dtype=f32)
        if state.ndim != 4 or state.shape[:2] != (2, 2) or state.shape[3] != self.spec.lstm_hidden:
            raise ValueError(f"a state has shape (2, 2, n, {self.spec.lstm_hidden}), not {state.shape}")
        _per_group(state.shape[2], self.groups)
        self._state = state

    def reset_state(self):
        if self._state is not None:
            self._state[...] = 0.0

    def _split(self, obs, episode_starts, final_obs):
        """Per group (rows of obs, of episode_starts, of final_obs or None, the lane slice)."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        n = obs.shape[0]
        m = _per_group(n, self.groups)
        starts = np.asarray(episode_starts).reshape(n)
        if final_obs is not None:
            final_obs = np.asarray(final_obs, dtype=f32).reshape(obs.shape)
        return n, [(obs[g * m:(g + 1) * m], starts[g * m:(g + 1) * m],
                    None if final_obs is None else final_obs[g * m:(g + 1) * m], slice(g * m, (g + 1) * m))
                   for g in range(self.groups)]

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, states=None):
        """(actions int64 [n], values, log_probs, final_values or None) over all n = G m rows: group g's rows by
        policies[g] from its columns of the state, which draws m of its own generator's numbers unless deterministic.  The
        population's own state advances in place, or -- with states=(in, out), two float32 [2, 2, n, H] arrays -- `out` is
        written from `in` and the own state stays."""
        n, pieces = self._split(obs, episode_starts, final_obs)
        source, target = (self._own_state(n),) * 2 if states is None else states
        parts = []
        for member, (rows, starts, final_rows, lanes) in zip(self.policies, pieces):
            before = np.ascontiguousarray(source[:, :, lanes, :])
            after = np.empty_like(before)
            parts.append(member.act(rows, starts, final_rows, deterministic, states=(before, after)))
            target[:, :, lanes, :] = after
        return tuple(None if parts[0][i] is None else np.concatenate([part[i] for part in parts]) for i in range(4))

    def values(self, obs, episode_starts, final_obs=None):
        """V(obs) from the own state masked by episode_starts; with final_obs (V(obs), V(final_obs)).  The state stays."""
        n, pieces = self._split(obs, episode_starts, final_obs)
        state = self._own_state(n)
        parts = []
        for member, (rows, starts, final_rows, lanes) in zip(self.policies, pieces):
            member.set_lstm_state(state[:, :, lanes, :])
            parts.append(member.values(rows, starts, final_rows))
        if final_obs is None:
            return np.concatenate(parts)
        return np.concatenate([part[0] for part in parts]), np.concatenate([part[1] for part in parts])


class LstmSdePopulationPolicy:
    """The numpy twin of DevicePopulationLstmSdePolicy, and its oracle: G lstm_sde.LstmSdePolicy, group g seeded with
    seeds[g], over slices of the lanes.  `params` is one array [G][P + L]; policies[g].params is its row g.  log_std_init: a
    scalar or G values, which override the spec's per group.  The state is ONE array [2, 2, n, H] as LstmPopulationPolicy's;
    num_envs (n = G m; reset_noise(num_envs=) sets it) says how many rows of noise a group draws: m L draws of its own
    generator per reset."""

    def __init__(self, spec, groups, seeds, log_std_init=None, num_envs=None):
        self.groups, seeds, inits = _checked_lstm_sde_population(spec, groups, seeds, log_std_init)
        self.spec = spec
        self.params = _initial_params(spec, inits)
        self._log_std_inits = inits
        self._state = None
        self.num_envs = self.groups
        if num_envs is not None:
            _per_group(int(num_envs), self.groups)
            self.num_envs = int(num_envs)
            self._state = np.zeros(spec.state_shape(num_envs), dtype=f32)
        self.policies = [lstm_sde_module.LstmSdePolicy(spec, seed, self.num_envs // self.groups) for seed in seeds]
        for g, member in enumerate(self.policies):
            member.params = self.params[g]

    _groups_of = PopulationPolicy._groups_of
    load_state_dict = PopulationPolicy.load_state_dict
    state_dict = PopulationPolicy.state_dict
    init_parameters = PopulationPolicy.init_parameters
    rng_state = PopulationPolicy.rng_state
    set_rng_state = PopulationPolicy.set_rng_state
    _own_state = LstmPopulationPolicy._own_state
    lstm_state = LstmPopulationPolicy.lstm_state
    set_lstm_state = LstmPopulationPolicy.set_lstm_state
    reset_state = LstmPopulationPolicy.reset_state
    _split = LstmPopulationPolicy._split
    values = LstmPopulationPolicy.values
    reset_noise = SdePopulationPolicy.reset_noise
    noise = SdePopulationPolicy.noise
    set_noise = SdePopulationPolicy.set_noise

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, states=None):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped)) over all
        n = G m rows: group g's rows by policies[g] from its columns of the state and its theta.  No draw is consumed.  The
        state advances as LstmPopulationPolicy.act's does."""
        n, pieces = self._split(obs, episode_starts, final_obs)
        if not deterministic:
            for member, (rows, _, _, _) in zip(self.policies, pieces):  # (before any group's state moves)
                theta = member.noise()
                if theta is None or theta.shape[0] != rows.shape[0]:
                    raise ValueError("a sampled act() needs reset_noise() of every group first")
        source, target = (self._own_state(n),) * 2 if states is None else states
        parts = []
        for member, (rows, starts, final_rows, lanes) in zip(self.policies, pieces):
            before = np.ascontiguousarray(source[:, :, lanes, :])
            after = np.empty_like(before)
            parts.append(member.act(rows, starts, final_rows, deterministic, states=(before, after)))
            target[:, :, lanes, :] = after
        return tuple(None if parts[0][i] is None else np.concatenate([part[i] for part in parts]) for i in range(5))


class PopulationLearner(_GroupHyper):
    """The numpy twin of DevicePopulationLearner, and its oracle: G learner.Learner, learners[g] over policies[g] and the
    group's rows.  With an LstmPopulationPolicy it is the recurrent learner: G lstm_learner.LstmLearner over slice-parts
    (group_parts), update(rollout_or_parts, firsts, count) and train(rollout, n_epochs, batch_size, splits, generator);
    with an LstmSdePopulationPolicy the same over float32 raw actions (the members' Gaussian head)."""

    def __init__(self, policy, learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, betas=(0.9, 0.999), adam_eps=1e-5):
        if not isinstance(policy, (PopulationPolicy, SdePopulationPolicy, LstmPopulationPolicy, LstmSdePopulationPolicy)):
            raise TypeError(f"PopulationLearner needs a PopulationPolicy, not {type(policy).__name__} (a "
                            "DevicePopulationPolicy has DevicePopulationLearner)")
        self.policy, self.spec, self.groups = policy, policy.spec, policy.groups
        self._lstm = self.spec.kind in RECURRENT_KINDS
        self._configure(learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps)
        member_learner = lstm_learner_module.LstmLearner if self._lstm else learner_module.Learner
        self.learners = [member_learner(member) for member in policy.policies]

    def _hand_down(self):
        for member, hyper in zip(self.learners, self.hypers()):
            member.learning_rate, member.clip_range, member.ent_coef, member.vf_coef = hyper[:4]
            member.max_grad_norm, member.betas, member.adam_eps = hyper.max_grad_norm, (hyper.beta1, hyper.beta2), hyper.adam_eps
            member.normalize_advantage = bool(hyper.normalize_advantage)

    def _pieces(self, flat):
        rows = _per_group(np.asarray(flat["actions"]).shape[0], self.groups)
        return rows, [{key: np.asarray(flat[key])[g * rows:(g + 1) * rows] for key in learner_module.BATCH_KEYS}
                      for g in range(self.groups)]

    def _recurrent_update(self, rollout_or_parts, firsts, count):
        parts = lstm_learner_module._parts(rollout_or_parts)
        rows = _per_group(int(parts["num_envs"]), self.groups) * int(parts["n_steps"])
        firsts = _checked_firsts(firsts, self.groups, rows)
        if not 1 <= int(count) <= min(rows, MAX_BATCH):
            raise ValueError(f"a minibatch of {count} rows is not in 1 .. {min(rows, MAX_BATCH)} (min(m T, {MAX_BATCH}))")
        self._hand_down()
        return np.stack([member.update(group_parts(parts, self.groups, g), firsts[g], int(count))
                         for g, member in enumerate(self.learners)])

    def _recurrent_train(self, rollout, n_epochs, batch_size, splits, generator):
        _refuse_rollout(self.spec, rollout)
        _refuse_other_groups(rollout, self.groups)
        parts = lstm_learner_module.parts_of(rollout)
        rows = _per_group(int(parts["num_envs"]), self.groups) * int(parts["n_steps"])
        n_epochs, batch_size, per_epoch = self._batches(rows, n_epochs, batch_size)
        splits = _group_splits(splits, n_epochs, self.groups, rows, generator)
        stats = np.zeros((n_epochs * per_epoch, self.groups, 8), dtype=f32)
        for epoch in range(n_epochs):
            for i in range(per_epoch):
                firsts = (splits[epoch] + i * batch_size) % rows
                stats[epoch * per_epoch + i] = self._recurrent_update(parts, firsts, min(batch_size, rows - i * batch_size))
        return stats

    def update(self, flat, index, count=None):
        """One minibatch update of every group: index int64 [G][B] of rows local to each group's piece of flat().
        Returns the stats float32 [G][8].  The recurrent learner: update(rollout_or_parts, firsts, count) -- G first rows,
        group g's minibatch is rows (firsts[g] + b) mod m T, b < count, of its own piece."""
        if self._lstm:
            if count is None:
                raise TypeError("the recurrent learner's update takes (rollout_or_parts, firsts, count)")
            return self._recurrent_update(flat, index, count)
        if count is not None:
            raise TypeError("count belongs to the recurrent learner's update(rollout_or_parts, firsts, count)")
        index = np.asarray(index, dtype=np.int64)
        if index.ndim != 2 or index.shape[0] != self.groups:
            raise ValueError(f"index has shape {index.shape}, not ({self.groups}, B)")
        rows, pieces = self._pieces(flat)
        if index.shape[1] > rows:
            raise ValueError(f"a minibatch of {index.shape[1]} is more than the {rows} rows of one group")
        self._hand_down()
        return np.stack([member.update(piece, index[g]) for g, (member, piece) in enumerate(zip(self.learners, pieces))])

    def train(self, rollout, n_epochs, batch_size, permutations=None, generator=None, splits=None):
        """n_epochs passes of every group over its rows of a finished rollout, in minibatches of batch_size (the last one
        may be shorter): stats float32 [n_epochs * ceil(m T / batch_size)][G][8].  Per epoch and group one permutation of
        the group's m T local rows: permutations[epoch][g] (int64 [n_epochs][G][m T]) if given, else
        generator.permutation(m T), drawn epoch by epoch and in group order.
        The recurrent learner: train(rollout, n_epochs, batch_size, splits=None, generator=None) -- the fourth argument is
        its splits, integers [n_epochs][G] in 0 .. m T - 1 (else generator.integers(m T, size=G) per epoch); per epoch and
        group the rows are rotated by the split and cut into consecutive minibatches, as lstm_learner.LstmLearner.train."""
        if self._lstm:
            if permutations is not None and splits is not None:
                raise TypeError("the recurrent learner takes its splits once (the fourth argument, or splits=)")
            return self._recurrent_train(rollout, n_epochs, batch_size, permutations if splits is None else splits, generator)
        if splits is not None:
            raise TypeError("splits belong to the recurrent learner; this one takes permutations")
        _refuse_rollout(self.spec, rollout)
        flat = rollout.flat()
        rows = _per_group(np.asarray(flat["actions"]).shape[0], self.groups)
        n_epochs, batch_size, per_epoch = self._batches(rows, n_epochs, batch_size)
        if permutations is not None:
            permutations = np.asarray(permutations, dtype=np.int64).reshape(n_epochs, self.groups, rows)
        elif generator is None:
            generator = np.random.default_rng()
        stats = np.zeros((n_epochs * per_epoch, self.groups, 8), dtype=f32)
        for epoch in range(n_epochs):
            order = permutations[epoch] if permutations is not None else np.stack(
                [generator.permutation(rows).astype(np.int64) for _ in range(self.groups)])
            for i in range(per_epoch):
                stats[epoch * per_epoch + i] = self.update(flat, order[:, i * batch_size:(i + 1) * batch_size])
        return stats

    def state_dict(self):
        """The G optimizers: lists step, bc1, bc2 and arrays m, v [G][P]."""
        parts = [member.state_dict() for member in self.learners]
        return {"step": [part["step"] for part in parts], "bc1": [part["bc1"] for part in parts],
                "bc2": [part["bc2"] for part in parts], "m": np.stack([part["m"] for part in parts]),
                "v": np.stack([part["v"] for part in parts])}

    def load_state_dict(self, state):
        for g, member in enumerate(self.learners):
            member.load_state_dict({"step": state["step"][g], "bc1": state["bc1"][g], "bc2": state["bc2"][g],
                                    "m": np.asarray(state["m"])[g], "v": np.asarray(state["v"])[g]})


class DevicePopulationPolicy:
    """The policies of G groups of m environments each of one device-resident environment (n = G m), over torch tensors on
    its GPU; used as PopulationPolicy is and bit for bit equal to it, group by group equal to a stand-alone
    DevicePolicy(seed=seeds[g]) over the group's m environments.

    Every act() / values() is ONE launch (rf_policy_forward_grouped), grid (ceil(m / 8), nets, G).  `params` is one
    float32 tensor [G][P].  The generators' words live in a device table written at seeding and at set_rng_state only;
    the number of draws each generator has given travels by value (every sampled act() takes m of each), so no call
    copies or waits.  rng_state() is computed on the host from the seeds and that count."""

    _device_env = policy_module.DevicePolicy._device_env
    _rows = policy_module.DevicePolicy._rows
    _out = policy_module.DevicePolicy._out

    def __init__(self, env, spec, groups, seeds):
        self._device_env(env)
        policy_module._refuse_box(env.single_action_space)
        self.groups, seeds = _checked_population(spec, groups, seeds)
        if env.single_action_space.n != spec.n_actions:
            raise ValueError(f"the spec has {spec.n_actions} actions, the environment {env.single_action_space.n}")
        self.num_envs = int(env.num_envs)
        self.per_group = _per_group(self.num_envs, self.groups)
        self._io = env._tensor_io()  # (ValueError, as step_tensors': a host initializer, a render_mode)
        from reinfocus_amd import torch_interop

        self._interop = torch_interop
        torch = self._torch = torch_interop._torch()
        self.spec = spec
        self._ctx = env._ctx
        self.device = torch.device("cuda", self._ctx.device)
        self.params = torch.zeros((self.groups, spec.size), dtype=torch.float32, device=self.device)
        self._owned = {}
        self._table = torch.zeros((self.groups, 4), dtype=torch.int64, device=self.device)  # (the bits of uint64 words)
        self._set_generators([np.random.PCG64DXSM(seed) for seed in seeds])

    def _set_generators(self, generators):
        self._generators, self._consumed = generators, 0
        words = np.array([policy_module.generator_words(generator) for generator in generators], dtype=np.uint64)
        self._table.copy_(self._torch.from_numpy(words.view(np.int64)))

    def rng_state(self):
        """What G stand-alone policies would return, in group order: each seed's generator advanced by the draws taken."""
        states = []
        for generator in self._generators:
            now = np.random.PCG64DXSM()
            now.state = generator.state
            states.append(now.advance(self._consumed).state)
        return states

    def set_rng_state(self, states):
        states = list(states)
        if len(states) != self.groups:
            raise ValueError(f"{len(states)} generator states for {self.groups} groups")
        generators = []
        for state in states:
            generator = np.random.PCG64DXSM()
            generator.state = state
            generators.append(generator)
        self._set_generators(generators)

    _groups_of = PopulationPolicy._groups_of

    def load_state_dict(self, state_dict, group=None):
        """Device tensors in SB3's names and shapes into group `group`, or into every group with None."""
        torch = self._torch
        groups = self._groups_of(group)
        for name in state_dict:
            tensor = state_dict[name]
            if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32:
                raise TypeError(f"{name} must be a torch.float32 tensor on {self.device}")
            self._io._on_device(tensor, name)
        with torch.no_grad():
            for name, at, shape, is_weight in self.spec.checked(state_dict, lambda t: t.shape):
                tensor = state_dict[name].detach()
                for g in groups:
                    self.params[g, at:at + tensor.numel()].view(shape).copy_(tensor.t() if is_weight else tensor)

    def init_parameters(self, seeds, ortho_init=True, groups=None):
        """PopulationPolicy.init_parameters on the device and bit for bit equal to it: rf_params_init over all G groups,
        two launches on torch's current stream whatever G is (one where nothing is orthogonal), into `params` in place.
        The seeds' generator words, the groups' log_std_init and the selection go up from pinned memory, stream-ordered;
        nothing waits for the host, and everything is checked before anything is enqueued."""
        from reinfocus_amd.environments import param_init

        param_init.init_device(self, self.params, seeds, ortho_init, groups, getattr(self, "_log_std_inits", None))

    def state_dict(self, group=0):
        """Group `group`'s parameters as device tensors in SB3's names and shapes (copies)."""
        row = self.params[self._groups_of(group)[0]]
        out = {}
        for name, at, shape, is_weight in self.spec.entries:
            view = row[at:at + int(np.prod(shape))].view(shape)
            out[name] = view.t().clone(memory_format=self._torch.contiguous_format) if is_weight else view.clone()
        return out

    def _all_rows(self, obs, final_obs):
        obs = self._rows(obs, "obs")
        if obs.shape[0] != self.num_envs:
            raise ValueError(f"obs has {obs.shape[0]} rows, the population {self.groups} groups of {self.per_group} "
                             f"environments ({self.num_envs})")
        if final_obs is not None and self._rows(final_obs, "final_obs").shape != obs.shape:
            raise ValueError(f"final_obs has shape {tuple(final_obs.shape)}, obs {tuple(obs.shape)}")
        return obs

    def _forward(self, obs, final_obs, sampled, flags, actions, log_probs, values, final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx.policy_forward_grouped(self.spec.desc(), self.groups, self.per_group, self.params.data_ptr(),
                                         obs.data_ptr(), pointer(final_obs), self._table.data_ptr() if sampled else None,
                                         self._consumed, flags, pointer(actions), pointer(log_probs), pointer(values),
                                         pointer(final_values), None, self._io._stream())

    def act(self, obs, final_obs=None, deterministic=False, out=None):
        """DevicePolicy.act over all n = G m rows, group g's rows with params[g] and its own generator.  One launch; a
        sampled call takes m draws of every generator."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        n = self.num_envs
        given = (None,) * 4 if out is None else tuple(out)
        if len(given) != 4:
            raise TypeError("out must be (actions, values, log_probs, final_values or None)")
        actions = self._out("actions", given[0], n, torch.int64)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        self._forward(obs, final_obs, not deterministic, DETERMINISTIC if deterministic else 0, actions, log_probs, values,
                      final_values)
        if not deterministic:
            self._consumed += self.per_group  # (after the call was taken: a refused call consumes nothing)
        return actions, values, log_probs, final_values

    def values(self, obs, final_obs=None, out=None):
        """DevicePolicy.values over all n rows.  One launch, no draw."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], self.num_envs, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], self.num_envs, torch.float32)
        self._forward(obs, final_obs, False, 0, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)


class DeviceSdePopulationPolicy:
    """The sde policies of G groups of m environments each of one device-resident environment with the Box(-1, 1, (1,))
    action space (n = G m), over torch tensors on its GPU; used as SdePopulationPolicy is and bit for bit equal to it,
    group by group equal to a stand-alone DeviceSdePolicy(seed=seeds[g]) over the group's m environments.

    reset_noise(groups=mask), act() and values() are ONE launch each (rf_sde_noise_reset_grouped, grid (ceil(m L / 256),
    G); rf_sde_forward_grouped, grid (ceil(m / 8), nets, G)).  `params` is one float32 tensor [G][P + L], theta one
    [G m][L].  The generators' words live in a device table written at seeding and at set_rng_state only.  The draws each
    generator has given are counted on the host (uint64 [G]); a reset sends them and the selection to the device from
    pinned memory, stream-ordered, so no call waits for the host.  rng_state() is computed on the host."""

    _device_env = policy_module.DevicePolicy._device_env
    _rows = policy_module.DevicePolicy._rows
    _out = policy_module.DevicePolicy._out

    def __init__(self, env, spec, groups, seeds, log_std_init=None):
        self._device_env(env)
        sde_module._refuse_discrete(env.single_action_space)
        self.groups, seeds, inits = _checked_sde_population(spec, groups, seeds, log_std_init)
        self.num_envs = int(env.num_envs)
        self.per_group = _per_group(self.num_envs, self.groups)
        self._io = env._tensor_io()  # (ValueError, as step_tensors': a host initializer, a render_mode)
        from reinfocus_amd import torch_interop

        self._interop = torch_interop
        torch = self._torch = torch_interop._torch()
        self.spec = spec
        self._ctx = env._ctx
        self.device = torch.device("cuda", self._ctx.device)
        self.params = torch.zeros((self.groups, spec.size), dtype=torch.float32, device=self.device)
        self.params.copy_(torch.from_numpy(_initial_params(spec, inits)))
        self._log_std_inits = inits
        self._owned = {}
        self._table = torch.zeros((self.groups, 4), dtype=torch.int64, device=self.device)  # (the bits of uint64 words)
        self._theta = torch.zeros((self.num_envs, spec.latent), dtype=torch.float32, device=self.device)
        self._has_noise = np.zeros(self.groups, dtype=bool)
        # what a reset reads on the device: uint64 [G] draws given, then uint8 [G] selected
        self._schedule = torch.zeros(9 * self.groups, dtype=torch.uint8, device=self.device)
        self._set_generators([np.random.PCG64DXSM(seed) for seed in seeds])

    def _set_generators(self, generators):
        self._generators, self._consumed = generators, np.zeros(self.groups, dtype=np.uint64)
        words = np.array([policy_module.generator_words(generator) for generator in generators], dtype=np.uint64)
        self._table.copy_(self._torch.from_numpy(words.view(np.int64)))

    def rng_state(self):
        """What G stand-alone policies would return, in group order: each seed's generator advanced by the draws taken."""
        states = []
        for generator, consumed in zip(self._generators, self._consumed):
            now = np.random.PCG64DXSM()
            now.state = generator.state
            states.append(now.advance(int(consumed)).state)
        return states

    set_rng_state = DevicePopulationPolicy.set_rng_state
    _groups_of = PopulationPolicy._groups_of
    load_state_dict = DevicePopulationPolicy.load_state_dict
    state_dict = DevicePopulationPolicy.state_dict
    init_parameters = DevicePopulationPolicy.init_parameters
    _all_rows = DevicePopulationPolicy._all_rows

    def reset_noise(self, groups=None, num_envs=None):
        """A new theta [m, L] for every selected group (None: every group; else a boolean sequence of length G) from the
        group's current log_std: ONE launch, and m L draws of each selected group's generator.  An unselected group keeps
        its rows of theta and its generator state."""
        torch = self._torch
        mask = group_mask(groups, self.groups)
        if num_envs is not None and int(num_envs) != self.num_envs:
            raise ValueError(f"num_envs {num_envs} is not the environment's {self.num_envs}")
        self._interop.check_one_runtime()
        G = self.groups
        packed = np.empty(9 * G, dtype=np.uint8)
        packed[:8 * G] = self._consumed.view(np.uint8)
        packed[8 * G:] = mask
        # (a pinned buffer of its own per call: the copy is stream-ordered, and resets enqueued before keep what they read)
        self._schedule.copy_(torch.from_numpy(packed).pin_memory(), non_blocking=True)
        at = self._schedule.data_ptr()
        self._ctx.sde_noise_reset_grouped(self.spec.desc(), G, self.per_group, self.params.data_ptr(),
                                          self._table.data_ptr(), at, None if groups is None else at + 8 * G,
                                          self._theta.data_ptr(), self._io._stream())
        self._consumed[mask] += np.uint64(self.per_group * self.spec.latent)  # (after the call was taken)
        self._has_noise |= mask

    def noise(self):
        """theta float32 [n, L] (a clone), or None while a group has none."""
        return self._theta.clone() if self._has_noise.all() else None

    def set_noise(self, theta):
        torch = self._torch
        if theta is None:
            self._has_noise[:] = False
            return
        if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 \
                or tuple(theta.shape) != (self.num_envs, self.spec.latent):
            raise ValueError(f"theta must be a torch.float32 tensor ({self.num_envs}, {self.spec.latent}) on {self.device}")
        self._io._on_device(theta, "theta")
        self._theta.copy_(theta)
        self._has_noise[:] = True

    def _forward(self, obs, final_obs, theta, flags, actions, env_actions, log_probs, values, final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx.sde_forward_grouped(self.spec.desc(), self.groups, self.per_group, self.params.data_ptr(), obs.data_ptr(),
                                      pointer(final_obs), pointer(theta), flags, pointer(actions), pointer(env_actions),
                                      pointer(log_probs), pointer(values), pointer(final_values), None, None,
                                      self._io._stream())

    def act(self, obs, final_obs=None, deterministic=False, out=None):
        """DeviceSdePolicy.act over all n = G m rows, group g's rows with params[g] and its rows of theta.  One launch; no
        draw is consumed."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        n = self.num_envs
        if not deterministic and not self._has_noise.all():
            raise ValueError("a sampled act() needs reset_noise() of every group first")
        given = (None,) * 5 if out is None else tuple(out)
        if len(given) != 5:
            raise TypeError("out must be (actions, values, log_probs, final_values or None, env_actions)")
        actions = self._out("raw_actions", given[0], n, torch.float32)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        env_actions = self._out("env_actions", given[4], n, torch.float32)
        self._forward(obs, final_obs, None if deterministic else self._theta,
                      DETERMINISTIC if deterministic else 0, actions, env_actions, log_probs, values, final_values)
        return actions, values, log_probs, final_values, env_actions

    def values(self, obs, final_obs=None, out=None):
        """DeviceSdePolicy.values over all n rows.  One launch, no draw."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], self.num_envs, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], self.num_envs, torch.float32)
        self._forward(obs, final_obs, None, 0, None, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)


class DevicePopulationLstmPolicy:
    """The recurrent policies of G groups of m environments each of one device-resident environment with a Discrete action
    space (n = G m), over torch tensors on its GPU; used as LstmPopulationPolicy is and bit for bit equal to it, group by
    group equal to a stand-alone lstm.DeviceLstmPolicy(seed=seeds[g]) over the group's m environments.  The spec is an
    LstmPolicySpec with either enable_critic_lstm.

    Every act() / values() is ONE launch (rf_lstm_forward_grouped), grid (ceil(m / 8), nets, G).  `params` is one float32
    tensor [G][P]; the state is one float32 [2, 2, n, H] tensor in DeviceLstmPolicy's form, which act() updates in place
    -- group g owns columns [g m, (g + 1) m) of each of its four planes.  The generators are DevicePopulationPolicy's: a
    device table of words written at seeding and at set_rng_state only, the draws taken travel by value.  Nothing waits
    for the host."""

    _device_env = policy_module.DevicePolicy._device_env
    _rows = policy_module.DevicePolicy._rows
    _out = policy_module.DevicePolicy._out

    def __init__(self, env, spec, groups, seeds):
        self._device_env(env)
        self.groups, seeds = _checked_lstm_population(spec, groups, seeds)
        if not hasattr(env.single_action_space, "n"):
            raise ValueError(f"a population of recurrent learners has a Categorical head over a Discrete action space, not "
                             f"{env.single_action_space!r}: the lstm-sde head in a population is out of scope here -- it is "
                             "the next step, DevicePopulationLstmSdePolicy")
        if env.single_action_space.n != spec.n_actions:
            raise ValueError(f"the spec has {spec.n_actions} actions, the environment {env.single_action_space.n}")
        self.num_envs = int(env.num_envs)
        self.per_group = _per_group(self.num_envs, self.groups)
        self._io = env._tensor_io()  # (ValueError, as step_tensors': a host initializer, a render_mode)
        from reinfocus_amd import torch_interop

        self._interop = torch_interop
        torch = self._torch = torch_interop._torch()
        self.spec = spec
        self._ctx = env._ctx
        self.device = torch.device("cuda", self._ctx.device)
        self.params = torch.zeros((self.groups, spec.size), dtype=torch.float32, device=self.device)
        self._owned = {}
        self._table = torch.zeros((self.groups, 4), dtype=torch.int64, device=self.device)  # (the bits of uint64 words)
        self._state = torch.zeros(spec.state_shape(self.num_envs), dtype=torch.float32, device=self.device)
        self._set_generators([np.random.PCG64DXSM(seed) for seed in seeds])

    _set_generators = DevicePopulationPolicy._set_generators
    rng_state = DevicePopulationPolicy.rng_state
    set_rng_state = DevicePopulationPolicy.set_rng_state
    _groups_of = PopulationPolicy._groups_of
    load_state_dict = DevicePopulationPolicy.load_state_dict
    state_dict = DevicePopulationPolicy.state_dict
    init_parameters = DevicePopulationPolicy.init_parameters
    _all_rows = DevicePopulationPolicy._all_rows
    _checked_state = lstm_module.DeviceLstmPolicy._checked_state
    lstm_state = lstm_module.DeviceLstmPolicy.lstm_state
    set_lstm_state = lstm_module.DeviceLstmPolicy.set_lstm_state
    reset_state = lstm_module.DeviceLstmPolicy.reset_state
    _starts = lstm_module.DeviceLstmPolicy._starts

    def _forward(self, obs, episode_starts, final_obs, state_in, state_out, sampled, flags, actions, log_probs, values,
                 final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx.lstm_forward_grouped(self.spec.critic_desc(), self.groups, self.per_group, self.params.data_ptr(),
                                       obs.data_ptr(), episode_starts.data_ptr(), pointer(final_obs), state_in.data_ptr(),
                                       pointer(state_out), self._table.data_ptr() if sampled else None, self._consumed,
                                       flags, pointer(actions), pointer(log_probs), pointer(values), pointer(final_values),
                                       None, self._io._stream())

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, out=None, states=None):
        """DeviceLstmPolicy.act over all n = G m rows, group g's rows with params[g], its own generator and its columns of
        the state.  The own state advances in place; with states=(in, out), two device tensors float32 [2, 2, n, H], the
        call goes from `in` to `out` instead (the same tensor, or two that do not overlap) and the own state stays.  One
        launch; a sampled call takes m draws of every generator."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        n = self.num_envs
        episode_starts = self._starts(episode_starts, n)
        if states is None:
            state_in = state_out = self._state
        else:
            state_in, state_out = states
            state_in, state_out = self._checked_state(state_in, "states[0]"), self._checked_state(state_out, "states[1]")
        given = (None,) * 4 if out is None else tuple(out)
        if len(given) != 4:
            raise TypeError("out must be (actions, values, log_probs, final_values or None)")
        actions = self._out("actions", given[0], n, torch.int64)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        self._forward(obs, episode_starts, final_obs, state_in, state_out, not deterministic,
                      DETERMINISTIC if deterministic else 0, actions, log_probs, values, final_values)
        if not deterministic:
            self._consumed += self.per_group  # (after the call was taken: a refused call consumes nothing)
        return actions, values, log_probs, final_values

    def values(self, obs, episode_starts, final_obs=None, out=None):
        """DeviceLstmPolicy.values over all n rows.  One launch, no draw; the state stays."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        episode_starts = self._starts(episode_starts, self.num_envs)
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], self.num_envs, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], self.num_envs, torch.float32)
        self._forward(obs, episode_starts, final_obs, self._state, None, False, 0, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)


class DevicePopulationLstmSdePolicy:
    """The recurrent sde policies of G groups of m environments each of one device-resident environment with the
    Box(-1, 1, (1,)) action space (n = G m), over torch tensors on its GPU; used as LstmSdePopulationPolicy is and bit for
    bit equal to it, group by group equal to a stand-alone lstm_sde.DeviceLstmSdePolicy(seed=seeds[g]) over the group's m
    environments.  The spec is an LstmSdePolicySpec with either enable_critic_lstm.

    reset_noise(groups=mask), act() and values() are ONE launch each (rf_lstm_sde_noise_reset_grouped, grid
    (ceil(m L / 256), G); rf_lstm_sde_forward_grouped, grid (ceil(m / 8), nets, G)).  `params` is one float32 tensor
    [G][P + L], theta one [G m][L], the state one [2, 2, n, H] in DeviceLstmPolicy's form, which act() updates in place.
    The generators are DeviceSdePopulationPolicy's: a device table of words written at seeding and at set_rng_state only,
    the draws each has given counted on the host and sent with the selection from pinned memory, stream-ordered.  Nothing
    waits for the host."""

    _device_env = policy_module.DevicePolicy._device_env
    _rows = policy_module.DevicePolicy._rows
    _out = policy_module.DevicePolicy._out

    def __init__(self, env, spec, groups, seeds, log_std_init=None):
        self._device_env(env)
        lstm_sde_module._refuse_discrete(env.single_action_space)
        self.groups, seeds, inits = _checked_lstm_sde_population(spec, groups, seeds, log_std_init)
        self.num_envs = int(env.num_envs)
        self.per_group = _per_group(self.num_envs, self.groups)
        self._io = env._tensor_io()  # (ValueError, as step_tensors': a host initializer, a render_mode)
        from reinfocus_amd import torch_interop

        self._interop = torch_interop
        torch = self._torch = torch_interop._torch()
        self.spec = spec
        self._ctx = env._ctx
        self.device = torch.device("cuda", self._ctx.device)
        self.params = torch.zeros((self.groups, spec.size), dtype=torch.float32, device=self.device)
        self.params.copy_(torch.from_numpy(_initial_params(spec, inits)))
        self._log_std_inits = inits
        self._owned = {}
        self._table = torch.zeros((self.groups, 4), dtype=torch.int64, device=self.device)  # (the bits of uint64 words)
        self._theta = torch.zeros((self.num_envs, spec.latent), dtype=torch.float32, device=self.device)
        self._state = torch.zeros(spec.state_shape(self.num_envs), dtype=torch.float32, device=self.device)
        self._has_noise = np.zeros(self.groups, dtype=bool)
        # what a reset reads on the device: uint64 [G] draws given, then uint8 [G] selected
        self._schedule = torch.zeros(9 * self.groups, dtype=torch.uint8, device=self.device)
        self._set_generators([np.random.PCG64DXSM(seed) for seed in seeds])

    _set_generators = DeviceSdePopulationPolicy._set_generators
    rng_state = DeviceSdePopulationPolicy.rng_state
    set_rng_state = DevicePopulationPolicy.set_rng_state
    _groups_of = PopulationPolicy._groups_of
    load_state_dict = DevicePopulationPolicy.load_state_dict
    state_dict = DevicePopulationPolicy.state_dict
    init_parameters = DevicePopulationPolicy.init_parameters
    _all_rows = DevicePopulationPolicy._all_rows
    _checked_state = lstm_module.DeviceLstmPolicy._checked_state
    lstm_state = lstm_module.DeviceLstmPolicy.lstm_state
    set_lstm_state = lstm_module.DeviceLstmPolicy.set_lstm_state
    reset_state = lstm_module.DeviceLstmPolicy.reset_state
    _starts = lstm_module.DeviceLstmPolicy._starts
    noise = DeviceSdePopulationPolicy.noise
    set_noise = DeviceSdePopulationPolicy.set_noise

    def reset_noise(self, groups=None, num_envs=None):
        """DeviceSdePopulationPolicy.reset_noise over this layout's log_std: ONE launch, and m L draws of each selected
        group's generator.  An unselected group keeps its rows of theta and its generator state."""
        torch = self._torch
        mask = group_mask(groups, self.groups)
        if num_envs is not None and int(num_envs) != self.num_envs:
            raise ValueError(f"num_envs {num_envs} is not the environment's {self.num_envs}")
        self._interop.check_one_runtime()
        G = self.groups
        packed = np.empty(9 * G, dtype=np.uint8)
        packed[:8 * G] = self._consumed.view(np.uint8)
        packed[8 * G:] = mask
        # (a pinned buffer of its own per call: the copy is stream-ordered, and resets enqueued before keep what they read)
        self._schedule.copy_(torch.from_numpy(packed).pin_memory(), non_blocking=True)
        at = self._schedule.data_ptr()
        self._ctx.lstm_sde_noise_reset_grouped(self.spec.critic_desc(), G, self.per_group, self.params.data_ptr(),
                                               self._table.data_ptr(), at, None if groups is None else at + 8 * G,
                                               self._theta.data_ptr(), self._io._stream())
        self._consumed[mask] += np.uint64(self.per_group * self.spec.latent)  # (after the call was taken)
        self._has_noise |= mask

    def _forward(self, obs, episode_starts, final_obs, state_in, state_out, theta, flags, actions, env_actions, log_probs,
                 values, final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx.lstm_sde_forward_grouped(self.spec.critic_desc(), self.groups, self.per_group, self.params.data_ptr(),
                                           obs.data_ptr(), episode_starts.data_ptr(), pointer(final_obs), state_in.data_ptr(),
                                           pointer(state_out), pointer(theta), flags, pointer(actions), pointer(env_actions),
                                           pointer(log_probs), pointer(values), pointer(final_values), None, None,
                                           self._io._stream())

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, out=None, states=None):
        """DeviceLstmSdePolicy.act over all n = G m rows, group g's rows with params[g], its rows of theta and its columns
        of the state.  The own state advances in place; with states=(in, out) the call goes from `in` to `out` instead and
        the own state stays.  One launch; no draw is consumed."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        n = self.num_envs
        episode_starts = self._starts(episode_starts, n)
        if not deterministic and not self._has_noise.all():
            raise ValueError("a sampled act() needs reset_noise() of every group first")
        if states is None:
            state_in = state_out = self._state
        else:
            state_in, state_out = states
            state_in, state_out = self._checked_state(state_in, "states[0]"), self._checked_state(state_out, "states[1]")
        given = (None,) * 5 if out is None else tuple(out)
        if len(given) != 5:
            raise TypeError("out must be (actions, values, log_probs, final_values or None, env_actions)")
        actions = self._out("raw_actions", given[0], n, torch.float32)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        env_actions = self._out("env_actions", given[4], n, torch.float32)
        self._forward(obs, episode_starts, final_obs, state_in, state_out, None if deterministic else self._theta,
                      DETERMINISTIC if deterministic else 0, actions, env_actions, log_probs, values, final_values)
        return actions, values, log_probs, final_values, env_actions

    def values(self, obs, episode_starts, final_obs=None, out=None):
        """DeviceLstmSdePolicy.values over all n rows.  One launch, no draw; the state stays."""
        torch = self._torch
        obs = self._all_rows(obs, final_obs)
        episode_starts = self._starts(episode_starts, self.num_envs)
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], self.num_envs, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], self.num_envs, torch.float32)
        self._forward(obs, episode_starts, final_obs, self._state, None, None, 0, None, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)


class DevicePopulationLearner(_GroupHyper):
    """The learners of a DevicePopulationPolicy or a DeviceSdePopulationPolicy, over torch tensors on its GPU; used as
    PopulationLearner is and bit for bit equal to it.  update() is rf_ppo_update_grouped (rf_sde_update_grouped with the
    Gaussian head, over float32 raw actions): three launches on torch's current stream whatever G is, which
    change policy.params in place.  The hyper-parameters are packed into one device tensor (G rf_ppo_hyper) when an
    update is enqueued, from pinned memory and only when they changed.  train() enqueues every update of every epoch back
    to back.  No method synchronises the host (state_dict() reads the steps and does).

    With a DevicePopulationLstmPolicy it is the recurrent learner: update(rollout_or_parts, firsts, count) and
    train(rollout, n_epochs, batch_size, splits, generator) as PopulationLearner's, rf_lstm_ppo_update_grouped -- six
    launches whatever G is; with a DevicePopulationLstmSdePolicy the same over float32 raw actions and P + L parameters
    (rf_lstm_sde_update_grouped).  The G first rows of every update are computed on the host and uploaded as one int32 table
    [updates][G] from pinned memory, stream-ordered."""

    def __init__(self, policy, learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, betas=(0.9, 0.999), adam_eps=1e-5):
        if not isinstance(policy, (DevicePopulationPolicy, DeviceSdePopulationPolicy, DevicePopulationLstmPolicy,
                                   DevicePopulationLstmSdePolicy)):
            raise TypeError(f"DevicePopulationLearner needs a DevicePopulationPolicy, not {type(policy).__name__} (a "
                            "PopulationPolicy has PopulationLearner, a DevicePolicy DeviceLearner)")
        self.policy, self.spec, self.groups = policy, policy.spec, policy.groups
        self._sde = self.spec.kind == sde_module.SdePolicySpec.kind
        self._lstm = self.spec.kind in RECURRENT_KINDS
        self._gaussian = self.spec.kind == LSTM_SDE_KIND  # (the recurrent learner over float32 raw actions)
        self._configure(learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps)
        self._torch, self._interop, self._io, self._ctx = policy._torch, policy._interop, policy._io, policy._ctx
        self.device = policy.device
        torch = self._torch
        self._state_floats = STATE_HEADER + 2 * self.spec.size
        if self._lstm:
            state_size = self._ctx.lstm_sde_grouped_state_size if self._gaussian else self._ctx.lstm_ppo_grouped_state_size
            state_bytes = state_size(self.spec.critic_desc(), self.groups, policy.per_group)
        else:
            state_size = self._ctx.sde_grouped_state_size if self._sde else self._ctx.ppo_grouped_state_size
            state_bytes = state_size(self.spec.desc(), self.groups, policy.per_group)
        if state_bytes != 4 * self.groups * self._state_floats:
            raise RuntimeError("rf_ppo_grouped_state_size / rf_sde_grouped_state_size / rf_lstm_ppo_grouped_state_size / "
                               "rf_lstm_sde_grouped_state_size disagrees with the packed optimizer states")
        self.state = torch.zeros((self.groups, self._state_floats), dtype=torch.float32, device=self.device)
        self._workspace, self._workspace_key = None, None
        self._stats = None
        self._hyper, self._hyper_key = None, None

    def _packed_hyper(self):
        """The device tensor of G rf_ppo_hyper (as float64 words: 8-byte aligned), rewritten when an attribute changed."""
        torch = self._torch
        hypers = self.hypers()
        key = tuple(hypers)
        if key != self._hyper_key:
            words = torch.from_numpy(hyper_records(hypers).view(f64).copy()).pin_memory()
            if self._hyper is None:
                self._hyper = torch.zeros(words.numel(), dtype=torch.float64, device=self.device)
            self._hyper.copy_(words, non_blocking=True)  # (stream-ordered: updates enqueued before keep what they read)
            self._hyper_key = key
        return self._hyper

    def _checked(self, flat, index):
        """(steps T, batch B) of flat() tensors of G m T rows and an index [G][B]."""
        torch = self._torch
        wanted = {"observations": torch.float32, "actions": torch.float32 if self._sde else torch.int64,
                  "log_probs": torch.float32, "advantages": torch.float32, "returns": torch.float32}
        total = None
        for key, dtype in wanted.items():
            tensor = flat[key]
            if not isinstance(tensor, torch.Tensor):
                raise TypeError(f"{key} must be a torch.Tensor on {self.device}, not {type(tensor).__name__}")
            self._io._on_device(tensor, key)
            shape = (tensor.shape[0], self.spec.obs_width) if key == "observations" else (tensor.shape[0],)
            if tensor.dtype != dtype or tuple(tensor.shape) != shape or not tensor.is_contiguous():
                raise ValueError(f"{key} is {tensor.dtype} {tuple(tensor.shape)}, not contiguous {dtype} {shape}")
            if total is not None and tensor.shape[0] != total:
                raise ValueError(f"{key} has {tensor.shape[0]} rows, the others {total}")
            total = tensor.shape[0]
        lanes = self.policy.num_envs
        if total < lanes or total % lanes != 0:
            raise ValueError(f"flat() has {total} rows, no multiple of the population's {lanes} environments")
        steps = total // lanes
        if not isinstance(index, torch.Tensor):
            raise TypeError(f"index must be a torch.Tensor on {self.device}, not {type(index).__name__}")
        self._io._on_device(index, "index")
        rows = steps * self.policy.per_group
        if index.dtype != torch.int64 or index.dim() != 2 or index.shape[0] != self.groups or not index.is_contiguous() \
                or not 1 <= index.shape[1] <= min(MAX_BATCH, rows):
            raise ValueError(f"index is {index.dtype} {tuple(index.shape)}, not contiguous torch.int64 ({self.groups}, "
                             f"1 .. {min(MAX_BATCH, rows)})")
        return steps, index.shape[1]

    def _room(self, steps, batch):
        key = (steps, batch)
        if key != self._workspace_key:
            if self._lstm:
                workspace_size = self._ctx.lstm_sde_grouped_workspace_size if self._gaussian \
                    else self._ctx.lstm_ppo_grouped_workspace_size
                size = workspace_size(self.spec.critic_desc(), self.groups, self.policy.per_group, steps, batch)
            else:
                workspace_size = self._ctx.sde_grouped_workspace_size if self._sde else self._ctx.ppo_grouped_workspace_size
                size = workspace_size(self.spec.desc(), self.groups, self.policy.per_group, steps, batch)
            if size == 0:
                raise RuntimeError(f"rf_ppo_grouped_workspace_size / rf_sde_grouped_workspace_size refuses minibatches of "
                                   f"{batch} out of {steps * self.policy.per_group} rows")
            if self._workspace is None or self._workspace.numel() < size // 4:
                self._workspace = self._torch.zeros(size // 4, dtype=self._torch.float32, device=self.device)
            self._workspace_key = key

    def _enqueue(self, flat, steps, index, stats, hyper):
        update = self._ctx.sde_update_grouped if self._sde else self._ctx.ppo_update_grouped
        update(self.spec.desc(), self.groups, self.policy.per_group, steps, hyper.data_ptr(), self.policy.params.data_ptr(),
               self.state.data_ptr(), self._workspace.data_ptr(), flat["observations"].data_ptr(),
               flat["actions"].data_ptr(), flat["log_probs"].data_ptr(), flat["advantages"].data_ptr(),
               flat["returns"].data_ptr(), index.shape[1], index.data_ptr(), stats.data_ptr(), self._io._stream())

    # ---- the recurrent learner (a DevicePopulationLstmPolicy) ---------------------------------------------------------
    def _own(self, rollout):
        if getattr(rollout, "device", None) != self.device:
            raise ValueError(f"the rollout lives on {getattr(rollout, 'device', 'the host')}, the policy on {self.device}")

    def _checked_parts(self, parts):
        """(steps T, rows m T of one group) of parts whose tensors are what rf_lstm_ppo_update_grouped reads."""
        torch = self._torch
        steps, lanes = int(parts["n_steps"]), int(parts["num_envs"])
        if steps < 1 or lanes != self.policy.num_envs:
            raise ValueError(f"the parts have n_steps {steps} and num_envs {lanes}; the population has "
                             f"{self.policy.num_envs} environments")
        total, hidden = steps * lanes, self.spec.lstm_hidden
        wanted = {"observations": (torch.float32, (total, self.spec.obs_width)),
                  "actions": (torch.float32 if self._gaussian else torch.int64, (total,)),
                  "log_probs": (torch.float32, (total,)), "advantages": (torch.float32, (total,)),
                  "returns": (torch.float32, (total,)), "episode_starts": (torch.uint8, (steps + 1, lanes)),
                  "lstm_states": (torch.float32, (steps + 1, 2, 2, lanes, hidden))}
        for key, (dtype, shape) in wanted.items():
            tensor = parts[key]
            if not isinstance(tensor, torch.Tensor):
                raise TypeError(f"{key} must be a torch.Tensor on {self.device}, not {type(tensor).__name__}")
            self._io._on_device(tensor, key)
            if tensor.dtype != dtype or tuple(tensor.shape) != shape or not tensor.is_contiguous():
                raise ValueError(f"{key} is {tensor.dtype} {tuple(tensor.shape)}, not contiguous {dtype} {shape}")
        return steps, steps * self.policy.per_group

    def _upload_firsts(self, table):
        """int [updates][G] as a device tensor int32, from pinned memory and stream-ordered: updates enqueued before keep
        what they read, and nothing waits for the host."""
        torch = self._torch
        host = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).pin_memory()
        return torch.empty(host.shape, dtype=torch.int32, device=self.device).copy_(host, non_blocking=True)

    def _enqueue_recurrent(self, parts, steps, firsts, count, stats, hyper):
        update = self._ctx.lstm_sde_update_grouped if self._gaussian else self._ctx.lstm_ppo_update_grouped
        update(
            self.spec.critic_desc(), self.groups, self.policy.per_group, steps, hyper.data_ptr(),
            self.policy.params.data_ptr(), self.state.data_ptr(), self._workspace.data_ptr(),
            parts["observations"].data_ptr(), parts["actions"].data_ptr(), parts["log_probs"].data_ptr(),
            parts["advantages"].data_ptr(), parts["returns"].data_ptr(), parts["episode_starts"].data_ptr(),
            parts["lstm_states"].data_ptr(), firsts.data_ptr(), count, stats.data_ptr(), self._io._stream())

    def _recurrent_update(self, rollout_or_parts, firsts, count):
        if hasattr(rollout_or_parts, "flat"):
            self._own(rollout_or_parts)
            _refuse_other_groups(rollout_or_parts, self.groups)
        parts = lstm_learner_module._parts(rollout_or_parts)
        steps, rows = self._checked_parts(parts)
        firsts = _checked_firsts(firsts, self.groups, rows)
        count = int(count)
        if not 1 <= count <= min(rows, MAX_BATCH):
            raise ValueError(f"a minibatch of {count} rows is not in 1 .. {min(rows, MAX_BATCH)} (min(m T, {MAX_BATCH}))")
        self._interop.check_one_runtime()
        self._room(steps, count)
        if self._stats is None:
            self._stats = self._torch.zeros((self.groups, 8), dtype=self._torch.float32, device=self.device)
        self._enqueue_recurrent(parts, steps, self._upload_firsts(firsts), count, self._stats, self._packed_hyper())
        return self._stats

    def _recurrent_train(self, rollout, n_epochs, batch_size, splits, generator):
        torch = self._torch
        _refuse_rollout(self.spec, rollout)
        self._own(rollout)
        _refuse_other_groups(rollout, self.groups)
        parts = lstm_learner_module.parts_of(rollout)
        steps, rows = self._checked_parts(parts)
        n_epochs, batch_size, per_epoch = self._batches(rows, n_epochs, batch_size)
        splits = _group_splits(splits, n_epochs, self.groups, rows, generator)
        # every update's G first rows, on the host: (split + i * batch_size) mod m T
        shifts = (np.arange(per_epoch, dtype=np.int64) * batch_size)[None, :, None]
        table = ((splits[:, None, :] + shifts) % rows).reshape(n_epochs * per_epoch, self.groups)
        self._interop.check_one_runtime()
        firsts = self._upload_firsts(table)
        hyper = self._packed_hyper()
        stats = torch.zeros((n_epochs * per_epoch, self.groups, 8), dtype=torch.float32, device=self.device)
        for update in range(n_epochs * per_epoch):
            i = update % per_epoch
            count = min(batch_size, rows - i * batch_size)
            self._room(steps, count)
            self._enqueue_recurrent(parts, steps, firsts[update], count, stats[update], hyper)
        return stats

    def update(self, flat, index, count=None):
        """One minibatch update of every group from rows index[g] (int64 device tensor [G][B], local to the group) of its
        piece of flat(); returns the stats, a float32 [G][8] tensor the learner owns and the next update() overwrites.
        The recurrent learner: update(rollout_or_parts, firsts, count) with G host integers as firsts."""
        if self._lstm:
            if count is None:
                raise TypeError("the recurrent learner's update takes (rollout_or_parts, firsts, count)")
            return self._recurrent_update(flat, index, count)
        if count is not None:
            raise TypeError("count belongs to the recurrent learner's update(rollout_or_parts, firsts, count)")
        steps, batch = self._checked(flat, index)
        self._interop.check_one_runtime()
        self._room(steps, batch)
        if self._stats is None:
            self._stats = self._torch.zeros((self.groups, 8), dtype=self._torch.float32, device=self.device)
        self._enqueue(flat, steps, index, self._stats, self._packed_hyper())
        return self._stats

    def train(self, rollout, n_epochs, batch_size, permutations=None, generator=None, splits=None):
        """As PopulationLearner.train, over a finished DeviceRollout of the policy's GPU: permutations is an int64 device
        tensor [n_epochs][G][m T] of local rows, else per epoch one device permutation per group (the argsort of one
        uniform draw [G][m T]; generator: a torch.Generator of that device).  Returns the stats as one device tensor
        [n_epochs * ceil(m T / batch_size)][G][8].  Nothing waits for the host.
        The recurrent learner: train(rollout, n_epochs, batch_size, splits=None, generator=None) -- the fourth argument is
        its splits, host integers [n_epochs][G] in 0 .. m T - 1 (else generator.integers(m T, size=G) per epoch of a
        numpy.random.Generator: a host draw costs no synchronisation)."""
        if self._lstm:
            if permutations is not None and splits is not None:
                raise TypeError("the recurrent learner takes its splits once (the fourth argument, or splits=)")
            return self._recurrent_train(rollout, n_epochs, batch_size, permutations if splits is None else splits, generator)
        if splits is not None:
            raise TypeError("splits belong to the recurrent learner; this one takes permutations")
        torch = self._torch
        _refuse_rollout(self.spec, rollout)
        if getattr(rollout, "device", None) != self.device:
            raise ValueError(f"the rollout lives on {getattr(rollout, 'device', 'the host')}, the policy on {self.device}")
        flat = rollout.flat()
        total = flat["actions"].shape[0]
        rows = _per_group(total, self.groups)
        n_epochs, batch_size, per_epoch = self._batches(rows, n_epochs, batch_size)
        if permutations is not None:
            if not isinstance(permutations, torch.Tensor) or permutations.dtype != torch.int64 \
                    or tuple(permutations.shape) != (n_epochs, self.groups, rows) or not permutations.is_contiguous():
                raise ValueError(f"permutations must be a contiguous torch.int64 tensor ({n_epochs}, {self.groups}, {rows})")
            self._io._on_device(permutations, "permutations")
        full = rows // batch_size

        def minibatches(order):
            """The epoch's index tensors [G][B], each contiguous: the full ones from one copy, then the short one."""
            cut = order[:, :full * batch_size].reshape(self.groups, full, batch_size).transpose(0, 1).contiguous()
            return [cut[i] for i in range(full)] + ([order[:, full * batch_size:].contiguous()] if per_epoch > full else [])

        first = minibatches(permutations[0] if permutations is not None
                            else torch.zeros((self.groups, rows), dtype=torch.int64, device=self.device))
        steps, _ = self._checked(flat, first[0])
        self._interop.check_one_runtime()
        hyper = self._packed_hyper()
        stats = torch.zeros((n_epochs * per_epoch, self.groups, 8), dtype=torch.float32, device=self.device)
        for epoch in range(n_epochs):
            if permutations is not None:
                batches = first if epoch == 0 else minibatches(permutations[epoch])
            else:
                batches = minibatches(torch.argsort(torch.rand((self.groups, rows), device=self.device,
                                                               generator=generator), dim=1))
            for i, index in enumerate(batches):
                self._room(steps, index.shape[1])
                self._enqueue(flat, steps, index, stats[epoch * per_epoch + i], hyper)
        return stats

    def state_dict(self):
        """The G optimizers: lists step, bc1, bc2 (read from the device: this synchronises) and clones of m, v [G][P]."""
        head = self.state[:, :STATE_HEADER].contiguous().cpu().numpy()
        size = self.spec.size
        return {"step": [int(row.view(np.int64)[0]) for row in head], "bc1": [float(row.view(f64)[1]) for row in head],
                "bc2": [float(row.view(f64)[2]) for row in head],
                "m": self.state[:, STATE_HEADER:STATE_HEADER + size].clone(), "v": self.state[:, STATE_HEADER + size:].clone()}

    def load_state_dict(self, state):
        torch = self._torch
        size = self.spec.size
        for key in ("m", "v"):
            tensor = state[key]
            if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32 or tensor.numel() != self.groups * size:
                raise ValueError(f"{key} must be a torch.float32 tensor ({self.groups}, {size}) on {self.device}")
            self._io._on_device(tensor, key)
        heads = np.stack([learner_module.pack_state(self.spec, int(state["step"][g]), float(state["bc1"][g]),
                                                    float(state["bc2"][g]), 0.0, 0.0)[:STATE_HEADER]
                          for g in range(self.groups)])
        self.state[:, :STATE_HEADER].copy_(torch.from_numpy(heads.copy()))
        self.state[:, STATE_HEADER:STATE_HEADER + size].copy_(state["m"].reshape(self.groups, size))
        self.state[:, STATE_HEADER + size:].copy_(state["v"].reshape(self.groups, size))
