"""CPU tests of the parameter initialisation (include/reinfocus_hip.h, "parameter init"; environments/param_init.py): the
numpy twin against the host build of csrc/rf_param_init.h (tests/paraminitcheck) as bytes, the uniform scheme's range and
moments, its bounds against PyTorch's own modules, the orthogonal scheme against float64 QR, the population twins, learning
from the initialisation, and the refusals.  tests/test_gpu_param_init.py holds the kernels to the same twin on the device."""

import ctypes

import numpy as np
import pytest

from reinfocus_amd.environments import harness
from reinfocus_amd.environments import param_init
from reinfocus_amd.environments.policy import generator_words
from tests import helpers
from tests import param_init_io_cases as cases

F32 = np.float32
bits = cases.bits


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(helpers.built("tests/paraminitcheck", "libparaminitcheck.so"))
    lib.pic_workspace_doubles.restype = ctypes.c_longlong
    return lib


def _pointer(array):
    return None if array is None else array.ctypes.data_as(ctypes.c_void_p)


def host_init(lib, table, stride, seeds, select=None, constants=None, fill=7.0):
    """pic_params_init over G groups on a sentinel-free array of `fill`; (params [G][stride], message or None)."""
    groups = len(seeds)
    array = param_init.segment_array(table)
    params = np.full((groups, stride), fill, dtype=F32)
    gens = np.array([generator_words(np.random.PCG64DXSM(seed)) for seed in seeds], dtype=np.uint64)
    select = None if select is None else np.asarray(select, dtype=np.uint8)
    constants = None if constants is None else np.asarray(constants, dtype=F32)
    message = ctypes.create_string_buffer(256)
    rc = lib.pic_params_init(array, len(table), groups, stride, _pointer(params), _pointer(gens), _pointer(select),
                             _pointer(constants), message, 256)
    return params, (message.value.decode() if rc else None)


# ---- 1: the twin is the host build, as bytes -----------------------------------------------------------------------------
@pytest.mark.parametrize("ortho_init", (False, True))
@pytest.mark.parametrize("name", sorted(cases.SMALL_SPECS))
def test_twin_equals_the_host_build(name, ortho_init, host):
    spec = cases.SMALL_SPECS[name]()
    table = param_init.segments(spec, ortho_init)
    constant = getattr(spec, "log_std_init", None)
    got, refused = host_init(host, table, spec.size, [cases.HIGH_SEED], constants=None if constant is None else [constant])
    assert refused is None
    want = param_init.init_numpy(spec, cases.HIGH_SEED, ortho_init)
    assert want.dtype == F32 and bits(got[0]) == bits(want)
    assert host.pic_workspace_doubles(param_init.segment_array(table), len(table), spec.size) == \
        2 * sum(out * in_ for _, out, in_, scheme, _ in table if scheme == param_init.ORTHOGONAL)


def test_twin_equals_the_host_build_at_full_width(host):
    """t = s = 256 and an in = 1 head input, both schemes (the orthogonal twin is shared with the tests below)."""
    spec = cases.wide_spec()
    for ortho_init in (False, True):
        got, refused = host_init(host, param_init.segments(spec, ortho_init), spec.size, [cases.WIDE_SEED])
        assert refused is None and bits(got[0]) == bits(cases.wide_twin(ortho_init))


def test_host_groups_select_and_positions_outside_every_segment(host):
    """G = 3 with a mask: group g equals the stand-alone run of seeds[g], an unselected group and the positions no segment
    covers keep their bytes."""
    spec = cases.SMALL_SPECS["sde"]()
    table = [row for row in param_init.segments(spec, True) if row[0] != 0]  # (the first weight is left out)
    hole = spec.entries[0][2][0] * spec.entries[0][2][1]
    inits = [-1.0, 0.5, 2.0]
    got, refused = host_init(host, table, spec.size, cases.SEEDS, select=[1, 0, 1], constants=inits)
    assert refused is None
    for g, seed in enumerate(cases.SEEDS):
        if g == 1:
            assert (got[g] == F32(7.0)).all()
            continue
        want = param_init.init_numpy(spec, seed, True, log_std_init=inits[g])
        assert (got[g, :hole] == F32(7.0)).all() and bits(got[g, hole:]) == bits(want[hole:])


# ---- 2: the uniform scheme -------------------------------------------------------------------------------------------------
def test_uniform_range_and_moments():
    """Every element of a UNIFORM segment lies in [-float32(scale), float32(scale)]; over the 256-wide arrays (N >= 4096)
    the mean is within 5 standard errors of 0 and the variance within 5 of scale^2 / 3.  Derived: a uniform variable on
    [-s, s] has variance s^2 / 3 and fourth moment s^4 / 5, so the mean of N has standard error s / sqrt(3 N) and the
    sample variance sqrt((1/5 - 1/9) / N) s^2."""
    checked = 0
    for spec, params in ((cases.wide_spec(), cases.wide_twin(False)),
                         (cases.SMALL_SPECS["lstm-sde"](), None), (cases.SMALL_SPECS["lstm-linear"](), None)):
        if params is None:
            params = param_init.init_numpy(spec, 11, False)
        for at, out, in_, scheme, scale in param_init.segments(spec, False):
            if scheme != param_init.UNIFORM:
                continue
            piece = params[at:at + out * in_]
            assert np.abs(piece).max() <= F32(scale)
            count = piece.size
            if count >= 4096:
                wide = piece.astype(np.float64)
                assert abs(wide.mean()) <= 5.0 * scale / np.sqrt(3.0 * count)
                assert abs(wide.var() - scale * scale / 3.0) <= 5.0 * np.sqrt((1.0 / 5.0 - 1.0 / 9.0) / count) * scale * scale
                checked += 1
    assert checked >= 2


# ---- 3: the bounds are PyTorch's ---------------------------------------------------------------------------------------------
def _scale_at(spec, name):
    """The UNIFORM scale of the segment that holds the first float of entry `name` under ortho_init=False."""
    offset = next(at for entry, at, _, _ in spec.entries if entry == name)
    for at, out, in_, scheme, scale in param_init.segments(spec, False):
        if at <= offset < at + out * in_:
            assert scheme == param_init.UNIFORM
            return scale
    raise AssertionError(name)


def test_uniform_bounds_are_pytorchs():
    """nn.Linear(in, out) and nn.LSTM(D, H) as torch initialises them: per array torch's max |w| is at most our scale, and at
    least 0.9 of it for the large arrays -- 1 / sqrt(in) for a Linear's weight and bias, 1 / sqrt(H) (not 1 / sqrt(D)) for
    every array of the LSTM, 1 / sqrt(D) for the linear critic.  stable-baselines3 is not needed for this; the gains of
    the orthogonal scheme are the documented ones (sqrt 2, 0.01, 1) and pinned by test_segments_of_every_spec."""
    import torch

    torch.manual_seed(5)
    width, hidden = 25, 64
    spec = harness.LstmPolicySpec(width, 7, lstm_hidden=hidden, pi=(64, 64), vf=(64,), enable_critic_lstm=False)
    lstm = torch.nn.LSTM(width, hidden)
    pairs = [(f"lstm_actor.{part}", getattr(lstm, part)) for part in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0",
                                                                       "bias_hh_l0")]
    critic, first, second, head = (torch.nn.Linear(width, hidden), torch.nn.Linear(hidden, 64), torch.nn.Linear(64, 64),
                                   torch.nn.Linear(64, 7))
    pairs += [("critic.weight", critic.weight), ("critic.bias", critic.bias),
              ("mlp_extractor.policy_net.0.weight", first.weight), ("mlp_extractor.policy_net.0.bias", first.bias),
              ("mlp_extractor.policy_net.2.weight", second.weight), ("mlp_extractor.policy_net.2.bias", second.bias),
              ("action_net.weight", head.weight), ("action_net.bias", head.bias)]
    large = 0
    for name, tensor in pairs:
        scale = _scale_at(spec, name)
        most = float(tensor.detach().abs().max())
        assert most <= scale, (name, most, scale)
        if tensor.numel() >= 1024:
            assert most >= 0.9 * scale, (name, most, scale)
            large += 1
    assert large >= 5
    assert _scale_at(spec, "lstm_actor.weight_ih_l0") == 1.0 / np.sqrt(64.0) != 1.0 / np.sqrt(25.0)
    assert _scale_at(spec, "critic.weight") == _scale_at(spec, "critic.bias") == 1.0 / np.sqrt(25.0)


def test_segments_of_every_spec():
    """The tables cover every spec kind exactly, within 32 segments at the largest network, with SB3's gains."""
    for make in list(cases.SMALL_SPECS.values()) + [cases.wide_spec, cases.widest_lstm_spec]:
        spec = make()
        for ortho_init in (False, True):
            table = param_init.segments(spec, ortho_init)
            assert len(table) <= param_init.MAX_SEGMENTS
            covered = np.zeros(spec.size, dtype=int)
            for at, out, in_, scheme, scale in table:
                assert 1 <= out <= 256 and 1 <= in_ <= 256
                covered[at:at + out * in_] += 1
            assert (covered == 1).all()
    spec = cases.SMALL_SPECS["lstm-sde-linear"]()
    by_offset = {row[0]: row for row in param_init.segments(spec, True)}
    for name, at, shape, is_weight in spec.entries:
        if name.startswith("lstm_actor."):
            continue
        row = by_offset[at]
        if name == "log_std":
            assert row[3] == param_init.CONSTANT
        elif name.startswith("critic."):
            assert row[3:] == (param_init.UNIFORM, 1.0 / np.sqrt(float(spec.obs_width)))
        elif not is_weight:
            assert row[3] == param_init.ZERO
        else:
            gain = np.sqrt(2.0) if name.startswith("mlp_extractor.") else 0.01 if name.startswith("action_net.") else 1.0
            assert row[1:] == (shape[1], shape[0], param_init.ORTHOGONAL, gain)


# ---- 4: orthogonality against float64 QR -------------------------------------------------------------------------------------
def _sign_fixed_qr(a):
    q, r = np.linalg.qr(a)
    return q * np.sign(np.diag(r))


def _orthogonal_figures(spec, params_seed):
    """Per orthogonal segment (shape, twin distance, float32-qr distance, twin max |Q^T Q - I|, float32-qr's)."""
    u = np.random.Generator(np.random.PCG64DXSM(params_seed)).random(spec.size)
    rows = []
    for at, out, in_, scheme, _ in param_init.segments(spec, True):
        if scheme != param_init.ORTHOGONAL:
            continue
        a = param_init.orthogonal_matrix(u[at:at + out * in_], out, in_)
        exact = _sign_fixed_qr(a.astype(np.float64))
        single = _sign_fixed_qr(a).astype(np.float64)
        twin = param_init.cgs2(a).astype(np.float64)
        eye = np.eye(a.shape[1])
        rows.append((a.shape, np.abs(twin - exact).max(), np.abs(single - exact).max(), np.abs(twin.T @ twin - eye).max(),
                     np.abs(single.T @ single - eye).max()))
    return rows


@pytest.mark.parametrize("name", ("mlp", "mlp-64", "mlp-256"))
def test_orthogonal_twin_against_float64_qr(name):
    """For each orthogonal segment: the twin's distance from the sign-fixed float64 QR of the same A, and max |Q^T Q - I|,
    are at most 16 x the same two quantities of numpy.linalg.qr run on A in float32.

    numpy.linalg.qr computes a float32 matrix in float64 and rounds the result once, so the baseline is half an ulp of each
    element.  With float32 chains the twin missed it from 64 x 64 on (88 x in distance at 64 x 64, 45 x and 39 x at
    256 x 256), and with float64 chains over vectors kept as float32 it still depended on the conditioning of A (46 x at
    256 x 256 for another seed); the definition therefore has float64 chains over float64 vectors and one rounding.
    Measured now (seed 1, printed below): at most 1.1 x in either quantity at every segment (profiles/param_init.md)."""
    spec = {"mlp": cases.SMALL_SPECS["mlp"], "mlp-64": cases.SMALL_SPECS["mlp-64"], "mlp-256": cases.wide_spec}[name]()
    rows = _orthogonal_figures(spec, 1)
    assert rows
    for row in rows:
        print("%s: distance twin %.3g float32 qr %.3g; orthogonality twin %.3g float32 qr %.3g" % row)
    for shape, twin_distance, single_distance, twin_orthogonality, single_orthogonality in rows:
        assert twin_distance <= 16.0 * single_distance, (shape, twin_distance, single_distance)
        assert twin_orthogonality <= 16.0 * single_orthogonality, (shape, twin_orthogonality, single_orthogonality)


def test_orthogonal_layout_and_gain():
    """W (SB3's [out][in]) has orthonormal rows where out < in and orthonormal columns otherwise, times the gain; the
    sign is torch's (positive diagonal of R): q_b . A[:, b] > 0."""
    spec = cases.SMALL_SPECS["mlp"]()
    state = spec.unpack(param_init.init_numpy(spec, 4, True))
    for name, gain in (("mlp_extractor.policy_net.0.weight", np.sqrt(2.0)), ("action_net.weight", 0.01),
                       ("value_net.weight", 1.0), ("mlp_extractor.value_net.2.weight", np.sqrt(2.0))):
        w = state[name].astype(np.float64) / gain
        gram = w @ w.T if w.shape[0] < w.shape[1] else w.T @ w
        assert np.abs(gram - np.eye(gram.shape[0])).max() < 1e-6, name
        assert (state[name.replace("weight", "bias")] == 0).all()
    a = param_init.orthogonal_matrix(np.random.default_rng(0).random(35), 7, 5)
    assert ((param_init.cgs2(a) * a).sum(axis=0) > 0).all()
    assert (param_init.cgs2(np.zeros((3, 2), dtype=F32)) == 0).all()  # (!(n2 > 0): the column is all zeros)


# ---- 5: the population twins -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ortho_init", (False, True))
@pytest.mark.parametrize("kind", cases.POPULATION_KINDS)
def test_population_twin_groups_are_stand_alone_twins(kind, ortho_init):
    make_spec, single_class, population_class, with_inits = cases.populations()[kind]
    spec = make_spec()
    inits = [-1.0, 0.5, 2.0]
    kw = dict(log_std_init=inits) if with_inits else {}
    population = population_class(spec, 3, [1, 2, 3], **kw)
    before = population.rng_state()
    population.init_parameters(cases.SEEDS, ortho_init)
    assert population.rng_state() == before and population.params.dtype == F32
    for g, seed in enumerate(cases.SEEDS):
        want = param_init.init_numpy(spec, seed, ortho_init, log_std_init=inits[g] if with_inits else None)
        assert bits(population.params[g]) == bits(want)
        assert bits(population.policies[g].params) == bits(want)
    # groups=: an unselected group keeps its bytes
    kept = population.params.copy()
    population.init_parameters([7, 8, 9], ortho_init, groups=[True, False, True])
    assert bits(population.params[1]) == bits(kept[1])
    assert bits(population.params[0]) != bits(kept[0]) and bits(population.params[2]) != bits(kept[2])
    assert bits(population.params[2]) == bits(param_init.init_numpy(spec, 9, ortho_init,
                                                                    log_std_init=inits[2] if with_inits else None))
    population.init_parameters([7, 8, 9], ortho_init, groups=[False, False, False])
    assert bits(population.params[1]) == bits(kept[1])
    # G = 1 is the ungrouped class
    one = population_class(spec, 1, [5])
    single = single_class(spec, 5)
    state = single.rng_state()
    one.init_parameters([cases.HIGH_SEED], ortho_init)
    single.init_parameters(cases.HIGH_SEED, ortho_init)
    assert bits(one.params[0]) == bits(single.params) and single.rng_state() == state
    assert bits(single.params) == bits(param_init.init_numpy(spec, cases.HIGH_SEED, ortho_init))


# ---- 6: learning from the initialisation ---------------------------------------------------------------------------------------
def _first_hidden(spec, params, name):
    return spec.unpack(params)[name]


def test_a_learner_learns_from_the_init_and_not_from_zeros():
    """Learner, m T = 32 rows, B = 16, two updates: from init_parameters(seed, ortho_init=False) the first hidden layer's
    weights differ from their initial bytes; from the constructor's zeros they are still all zero."""
    spec = harness.MlpPolicySpec(4, 3, pi=(6,), vf=(5,))
    rng = np.random.default_rng(3)
    flat = {"observations": rng.standard_normal((32, 4)).astype(F32), "actions": rng.integers(0, 3, 32).astype(np.int64),
            "log_probs": (-1.1 + 0.1 * rng.standard_normal(32)).astype(F32),
            "advantages": rng.standard_normal(32).astype(F32), "returns": rng.standard_normal(32).astype(F32)}
    names = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.value_net.0.weight")
    for initialised in (True, False):
        policy = harness.Policy(spec, 0)
        if initialised:
            policy.init_parameters(21, ortho_init=False)
        first = policy.params.copy()
        learner = harness.Learner(policy, learning_rate=1e-2)
        for update in range(2):
            learner.update(flat, np.arange(16 * update, 16 * update + 16))
        for name in names:
            now, then = _first_hidden(spec, policy.params, name), _first_hidden(spec, first, name)
            if initialised:
                assert bits(now) != bits(then) and np.abs(now - then).max() > 1e-4, name
            else:
                assert (now == 0).all() and (then == 0).all(), name


def test_a_recurrent_learner_learns_from_the_init_and_not_from_zeros():
    """The same for LstmLearner at H = 4 (T = 8, m = 4): W_ih and W_hh of both LSTMs move from the init, stay zero from zeros."""
    spec = harness.LstmPolicySpec(3, 2, lstm_hidden=4, pi=(5,), vf=(5,))
    rng = np.random.default_rng(4)
    steps, lanes = 8, 4
    total = steps * lanes
    starts = np.zeros((steps + 1, lanes), dtype=np.uint8)
    starts[0] = 1
    starts[5, 2] = 1
    parts = {"observations": rng.standard_normal((total, 3)).astype(F32), "actions": rng.integers(0, 2, total).astype(np.int64),
             "log_probs": (-0.7 + 0.1 * rng.standard_normal(total)).astype(F32),
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32),
             "episode_starts": starts, "lstm_states": (0.5 * rng.standard_normal((steps + 1,) + spec.state_shape(lanes))).astype(F32),
             "n_steps": steps, "num_envs": lanes}
    names = ("lstm_actor.weight_ih_l0", "lstm_actor.weight_hh_l0", "lstm_critic.weight_ih_l0", "lstm_critic.weight_hh_l0")
    for initialised in (True, False):
        policy = harness.LstmPolicy(spec, 0)
        if initialised:
            policy.init_parameters(22, ortho_init=False)
        first = policy.params.copy()
        learner = harness.LstmLearner(policy, learning_rate=1e-2)
        for update in range(2):
            learner.update(parts, 16 * update, 16)
        for name in names:
            now, then = _first_hidden(spec, policy.params, name), _first_hidden(spec, first, name)
            if initialised:
                assert bits(now) != bits(then), name
            else:
                assert (now == 0).all() and (then == 0).all(), name


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------
def test_the_table_refusals(host):
    """What rf_params_init refuses of a table, each with a message (csrc/rf_param_init.h param_table, which the entry point
    reports): more than 32 segments, overlapping and out-of-range segments, an unknown scheme, a non-finite or
    non-positive scale of UNIFORM / ORTHOGONAL, CONSTANT without constants; and a width outside the limits."""
    U, O, C, Z = param_init.UNIFORM, param_init.ORTHOGONAL, param_init.CONSTANT, param_init.ZERO
    good = [(0, 4, 3, U, 0.5), (12, 4, 1, Z, 0.0), (16, 2, 4, O, 1.0)]
    assert host_init(host, good, 24, [1])[1] is None
    many = [(i, 1, 1, Z, 0.0) for i in range(33)]
    assert "more segments" in host_init(host, many, 64, [1])[1]
    assert host_init(host, many[:32], 64, [1])[1] is None
    assert "overlap" in host_init(host, [(0, 4, 3, U, 0.5), (11, 4, 1, Z, 0.0)], 24, [1])[1]
    assert "overlap" in host_init(host, [(4, 2, 2, Z, 0.0), (0, 4, 3, U, 0.5)], 24, [1])[1]
    assert "out of range" in host_init(host, [(0, 4, 3, U, 0.5), (21, 4, 1, Z, 0.0)], 24, [1])[1]
    assert "out of range" in host_init(host, [(2 ** 32 - 2, 2, 2, Z, 0.0)], 24, [1])[1]
    assert "unknown" in host_init(host, [(0, 4, 3, 4, 0.5)], 24, [1])[1]
    assert "unknown" in host_init(host, [(0, 4, 3, -1, 0.5)], 24, [1])[1]
    for scheme in (U, O):
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            assert "scale" in host_init(host, [(0, 4, 3, scheme, scale)], 24, [1])[1], (scheme, scale)
    assert host_init(host, [(0, 4, 3, Z, float("nan"))], 24, [1])[1] is None  # (unused: not looked at)
    assert "d_constants" in host_init(host, [(0, 4, 1, C, 0.0)], 24, [1])[1]
    assert host_init(host, [(0, 4, 1, C, 0.0)], 24, [1], constants=[2.0])[1] is None
    for out, in_ in ((0, 1), (1, 0), (257, 1), (1, 257), (-1, 1)):
        assert "RF_POLICY_MAX_WIDTH" in host_init(host, [(0, out, in_, Z, 0.0)], 70000, [1])[1]
    untouched, refused = host_init(host, [(0, 4, 3, U, 0.5), (11, 4, 1, Z, 0.0)], 24, [1])
    assert refused and (untouched == F32(7.0)).all()


def test_the_classes_refusals():
    """A wrong number of seeds, a mask of the wrong length and a non-boolean ortho_init are refused with a message, and the
    parameters keep their bytes."""
    spec = cases.SMALL_SPECS["mlp"]()
    population = harness.PopulationPolicy(spec, 3, [1, 2, 3])
    population.init_parameters([4, 5, 6], False)
    kept = population.params.copy()
    with pytest.raises(ValueError, match="one seed per group"):
        population.init_parameters([1, 2], False)
    with pytest.raises(ValueError, match="one seed per group"):
        population.init_parameters(5, False)
    with pytest.raises(ValueError, match="one entry per group"):
        population.init_parameters([1, 2, 3], False, groups=[True, False])
    with pytest.raises(ValueError, match="one entry per group"):
        population.init_parameters([1, 2, 3], False, groups=[1.0, 0.0, 1.0])
    for wrong in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError, match="ortho_init"):
            population.init_parameters([1, 2, 3], wrong)
        with pytest.raises(TypeError, match="ortho_init"):
            harness.Policy(spec, 0).init_parameters(1, wrong)
    assert bits(population.params) == bits(kept)


def test_the_public_surface():
    """init_parameters on all sixteen classes, exported through harness with the twin's functions."""
    for name in ("Policy", "SdePolicy", "LstmPolicy", "LstmSdePolicy", "DevicePolicy", "DeviceSdePolicy", "DeviceLstmPolicy",
                 "DeviceLstmSdePolicy", "PopulationPolicy", "SdePopulationPolicy", "LstmPopulationPolicy",
                 "LstmSdePopulationPolicy", "DevicePopulationPolicy", "DeviceSdePopulationPolicy",
                 "DevicePopulationLstmPolicy", "DevicePopulationLstmSdePolicy"):
        assert callable(getattr(getattr(harness, name), "init_parameters")), name
    assert harness.init_numpy is param_init.init_numpy and harness.segments is param_init.segments
    assert (harness.Policy(cases.SMALL_SPECS["mlp"](), 0).params == 0).all()  # (the constructors still give zeros)
