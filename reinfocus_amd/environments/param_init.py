"""The initialisation of a learner's packed parameters, as stable-baselines3 does it, per group on the device.

Every policy class here starts at zero, and from zero no net learns anything but its head biases: hidden activations are
0, so the gradient of every head weight is 0, so every delta handed back is 0.  init_parameters(seed, ortho_init) of the
policy classes is the step between a constructor and training.

One definition (include/reinfocus_hip.h, "parameter init"): a packed array is a table of segments, each ZERO, CONSTANT,
UNIFORM (PyTorch's default, (2 u - 1) / sqrt(fan)) or ORTHOGONAL (torch.nn.init.orthogonal_ by Gram-Schmidt done twice in
a fixed float64 order, rounded once); packed position i uses draw number i of numpy's Generator(PCG64DXSM(seed)).  init_numpy below is
its numpy float32 restatement and the oracle; param_fill_kernel and param_orthogonal_kernel (csrc/rf_param_init.h)
compute the same bits in two launches for all G groups of a population (rf_params_init).

    segments(spec, ortho_init)    the table of a spec, from the spec's own entries (all five spec kinds)
    init_numpy(spec, seed, ...)   the packed float32 vector
    init_twin / init_device       what the policy classes' init_parameters call (one learner is a population of one)

ortho_init=False is what the reference's tuned configurations and every trial of its search use: every array UNIFORM with
PyTorch's fans -- an nn.Linear(in, out) weight and bias fan = in, every array of an nn.LSTM(D, H) fan = H, the linear
critic nn.Linear(D, H) fan = D.  ortho_init=True is SB3's default: mlp_extractor weights ORTHOGONAL with gain sqrt 2,
action_net 0.01, value_net 1, their biases ZERO; the LSTMs and the linear critic keep PyTorch's default (sb3-contrib
creates them after _build).  log_std is CONSTANT (log_std_init) in both.

Deliberate differences from SB3: the project's generator and normal32, not torch's global RNG; CGS2 in a fixed
order, not LAPACK's QR; one seed per group; draws indexed by position.
"""

import ctypes

import numpy as np

from reinfocus_amd.environments.policy import MAX_WIDTH, f32, generator_words
from reinfocus_amd.environments.sde import normal32

ZERO, CONSTANT, UNIFORM, ORTHOGONAL = 0, 1, 2, 3  # RF_INIT_*
MAX_SEGMENTS = 32  # RF_PARAM_MAX_SEGMENTS
GAIN_EXTRACTOR, GAIN_ACTION, GAIN_VALUE = float(np.sqrt(2.0)), 0.01, 1.0  # SB3's ActorCriticPolicy._build


class ParamSegment(ctypes.Structure):
    """rf_param_segment (include/reinfocus_hip.h)."""

    _fields_ = [("at", ctypes.c_uint), ("out", ctypes.c_int), ("in_", ctypes.c_int), ("scheme", ctypes.c_int),
                ("scale", ctypes.c_double)]


def uniform_scale(fan):
    """1.0 / sqrt(float64(fan)): the bound of PyTorch's default initialisation."""
    return 1.0 / float(np.sqrt(np.float64(fan)))


def checked_ortho_init(ortho_init):
    if not isinstance(ortho_init, (bool, np.bool_)):
        raise TypeError(f"ortho_init must be True or False, not {ortho_init!r}")
    return bool(ortho_init)


def _runs(at, rows, width, scale):
    """A run of rows x width floats of one UNIFORM scale as segments of out = width and at most MAX_WIDTH rows each."""
    out = []
    while rows > 0:
        take = min(rows, MAX_WIDTH)
        out.append((at, width, take, UNIFORM, scale))
        at += take * width
        rows -= take
    return out


def segments(spec, ortho_init):
    """The table of `spec` (MlpPolicySpec, SdePolicySpec, LstmPolicySpec with either critic, LstmSdePolicySpec alike): a
    list of (at, out, in, scheme, scale) that covers the packed vector exactly.  The four arrays of an LSTM are one run of
    4 (D + H + 2) rows of H floats with one scale, cut into segments of at most 256 rows (I1 of "parameter init")."""
    ortho_init = checked_ortho_init(ortho_init)
    table, fan_in, lstm_parts = [], None, 0
    hidden = getattr(spec, "lstm_hidden", None)
    for name, at, shape, is_weight in spec.entries:
        if name.startswith(("lstm_actor.", "lstm_critic.")):
            if lstm_parts == 0:  # (weight_ih_l0: the run starts here and takes the three arrays after it)
                table.extend(_runs(at, 4 * (spec.obs_width + hidden + 2), hidden, uniform_scale(hidden)))
            lstm_parts = (lstm_parts + 1) % 4
            continue
        if name == "log_std":
            table.append((at, shape[1], 1, CONSTANT, 0.0))
            continue
        linear_critic = name.startswith("critic.")
        if name.endswith(".weight"):
            fan_in, out = shape
            if ortho_init and not linear_critic:
                gain = GAIN_EXTRACTOR if name.startswith("mlp_extractor.") else \
                    GAIN_ACTION if name.startswith("action_net.") else GAIN_VALUE
                table.append((at, out, fan_in, ORTHOGONAL, gain))
            else:
                table.append((at, out, fan_in, UNIFORM, uniform_scale(fan_in)))
        elif ortho_init and not linear_critic:
            table.append((at, shape[0], 1, ZERO, 0.0))
        else:  # (a bias follows its weight: the fan is the weight's)
            table.append((at, shape[0], 1, UNIFORM, uniform_scale(fan_in)))
    assert len(table) <= MAX_SEGMENTS and sum(s[1] * s[2] for s in table) == spec.size, (len(table), spec.size)
    return table


def segment_array(table):
    """The ctypes array of rf_param_segment of a table."""
    return (ParamSegment * len(table))(*[ParamSegment(*row) for row in table])


def cgs2(a):
    """The Q float32 [t, s] of a float32 [t, s] (t >= s), I5 of "parameter init" literally: every chain in float64, from +0,
    ascending, a multiply then an add; the finished vectors stay float64 and are rounded to float32 once, at the end."""
    a = np.asarray(a, dtype=f32)
    t, s = a.shape
    q = np.zeros((t, s), dtype=np.float64)
    with np.errstate(all="ignore"):
        for b in range(s):
            v = a[:, b].astype(np.float64)
            for _ in range(2):
                c = np.zeros(b, dtype=np.float64)
                for i in range(t):
                    c = c + q[i, :b] * v[i]
                for p in range(b):
                    v = v - c[p] * q[:, p]
            n2 = np.float64(0.0)
            for x in v:
                n2 = n2 + x * x
            if n2 > 0.0:
                q[:, b] = v / np.sqrt(n2)
    return q.astype(f32)


def orthogonal_matrix(u, out, in_):
    """A [t, s] of an orthogonal segment: normal32 of its out * in draws."""
    return normal32(u).reshape(max(out, in_), min(out, in_))


def orthogonal_numpy(u, out, in_, gain):
    """The packed out * in floats (W^T [in][out]) of an ORTHOGONAL segment from its draws u float64 [out * in]."""
    q = cgs2(orthogonal_matrix(u, out, in_))
    # out >= in: W^T[k][j] = q_k[j], the transpose of Q [out][in]; out < in: W^T[k][j] = q_j[k], Q [in][out] itself
    packed = q.T if out >= in_ else q
    return (f32(gain) * np.ascontiguousarray(packed)).reshape(-1)


def fill_numpy(table, size, seed, constant=None, out=None):
    """The packed float32 [size] of a table for one group: draw number i of Generator(PCG64DXSM(seed)) for position i.
    `out`: written in place (positions outside every segment stay)."""
    u = np.random.Generator(np.random.PCG64DXSM(seed)).random(size)
    params = np.zeros(size, dtype=f32) if out is None else out
    for at, width, rows, scheme, scale in table:
        cells = width * rows
        if scheme == ZERO:
            params[at:at + cells] = f32(0.0)
        elif scheme == CONSTANT:
            if constant is None:
                raise ValueError("a CONSTANT segment needs its constant")
            params[at:at + cells] = f32(constant)
        elif scheme == UNIFORM:
            params[at:at + cells] = ((2.0 * u[at:at + cells] - 1.0) * scale).astype(f32)
        elif scheme == ORTHOGONAL:
            params[at:at + cells] = orthogonal_numpy(u[at:at + cells], width, rows, scale)
        else:
            raise ValueError(f"unknown scheme {scheme}")
    return params


def init_numpy(spec, seed, ortho_init, log_std_init=None, out=None):
    """The numpy twin of rf_params_init for one group: the packed float32 vector of `spec`."""
    if log_std_init is None:
        log_std_init = getattr(spec, "log_std_init", None)
    return fill_numpy(segments(spec, ortho_init), spec.size, seed, log_std_init, out)


def _checked_seeds(seeds, groups):
    seeds = list(seeds) if isinstance(seeds, (list, tuple, np.ndarray)) else None
    if seeds is None or len(seeds) != groups:
        raise ValueError(f"seeds must be a sequence of one seed per group ({groups}), not "
                         f"{'a scalar' if seeds is None else len(seeds)}")
    return seeds


def _checked_mask(selected, groups):
    from reinfocus_amd.environments import population

    return None if selected is None else population.group_mask(selected, groups)


def init_twin(params, spec, seeds, ortho_init, selected=None, constants=None):
    """init_parameters of the numpy classes: rows of params float32 [G][size] in place, group g from seeds[g] (and
    constants[g], its log_std_init), the groups of `selected` only."""
    table = segments(spec, ortho_init)
    groups = params.shape[0]
    seeds = _checked_seeds(seeds, groups)
    mask = _checked_mask(selected, groups)
    for g in range(groups):
        if mask is None or mask[g]:
            constant = getattr(spec, "log_std_init", None) if constants is None else constants[g]
            fill_numpy(table, spec.size, seeds[g], constant, out=params[g])


def init_device(owner, params, seeds, ortho_init, selected=None, constants=None):
    """init_parameters of the device classes: rf_params_init over params (a float32 tensor [G][size] or [size]) on
    torch's current stream -- two launches.  The generators' words, the constants and the selection go up from pinned
    memory in one stream-ordered copy, as reset_noise's schedule does; nothing waits for the host.  Everything is checked
    before anything is enqueued."""
    torch, spec = owner._torch, owner.spec
    table = segments(spec, ortho_init)
    groups = 1 if params.dim() == 1 else params.shape[0]
    seeds = _checked_seeds(seeds, groups)
    mask = _checked_mask(selected, groups)
    if constants is None and hasattr(spec, "log_std_init"):
        constants = [spec.log_std_init] * groups
    owner._interop.check_one_runtime()
    array = segment_array(table)
    # what the kernels read on the device: uint64 [G][4] generator words, float32 [G] constants, uint8 [G] selected
    packed = np.zeros(37 * groups, dtype=np.uint8)
    words = np.array([generator_words(np.random.PCG64DXSM(seed)) for seed in seeds], dtype=np.uint64)
    packed[:32 * groups] = words.reshape(-1).view(np.uint8)
    if constants is not None:
        packed[32 * groups:36 * groups] = np.array([float(x) for x in constants], dtype=f32).view(np.uint8)
    packed[36 * groups:] = 1 if mask is None else mask
    stage = getattr(owner, "_init_stage", None)
    if stage is None:
        stage = owner._init_stage = torch.zeros(37 * groups, dtype=torch.uint8, device=owner.device)
        owner._init_workspace = {}  # (by size: one per scheme)
    need = owner._ctx.params_init_workspace_size(array, len(table), groups)
    workspace = owner._init_workspace.get(need)
    if workspace is None and need:
        workspace = owner._init_workspace[need] = torch.empty(need // 8, dtype=torch.float64, device=owner.device)
    # (a pinned buffer of its own per call: the copy is stream-ordered, and calls enqueued before keep what they read)
    stage.copy_(torch.from_numpy(packed).pin_memory(), non_blocking=True)
    at = stage.data_ptr()
    owner._ctx.params_init(array, len(table), groups, spec.size, params.data_ptr(), at,
                           None if mask is None else at + 36 * groups, None if constants is None else at + 32 * groups,
                           None if workspace is None else workspace.data_ptr(), owner._io._stream())
