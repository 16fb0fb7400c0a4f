"""Compiles strategy objects into the device program of a composed environment (rf_env_program, rf_env_configure_composed).

A program holds the transformer (its kind and parameters), up to eight ender leaves with a postfix list of `|` / `&`
over them, and up to eight rewarder leaves with a postfix list of `+` / `*` and the dtype of every node.  Leaves are
numbered in the order a left-to-right walk of the tree meets them; that is also the order of the per-leaf strategy
state the device keeps (rf_env_get_strategy_state) and `host_strategy_state` reads from the host twin's objects.

An observer tree is compiled into a second, separate program (rf_env_observer_program, rf_env_configure_observed):
its nodes in evaluation order -- children before their wrapper, left to right -- over a stack of float32 columns (see
`compile_observer`).  The DeltaObservers' old values are kept node-major in that order (rf_env_get_observer_state,
`host_observer_state`).

Every check of rf_env_configure_composed / rf_env_configure_observed is made here first and raises AssertionError, so that nothing malformed
reaches the device; so do the checks only Python can make: every strategy's num_envs, and rewarders whose numpy result
would not be floating point (an OnTargetRewarder with integer on / off, which numpy evaluates in int64) or not in the
dtype the device computes them in (an OnTargetRewarder / StoppedRewarder with numpy.float32 on and off / reward).
"""

import math

import numpy as np

from reinfocus_amd import _native
from reinfocus_amd.environments import episode_ender
from reinfocus_amd.environments import episode_rewarder
from reinfocus_amd.environments import scalars
from reinfocus_amd.environments import state_initializer
from reinfocus_amd.environments import state_observer
from reinfocus_amd.environments import state_transformer

# the dtype numpy 1.26 gives each rewarder leaf with Python-number or numpy.float64 parameters (environments/scalars.py),
# which is the one the device computes it in; numpy.float32 on / off or reward make OnTarget / Stopped float32: refused
LEAF_DTYPES = {
    episode_rewarder.DELTA: np.dtype(np.float32),
    episode_rewarder.DISTANCE: np.dtype(np.float32),
    episode_rewarder.OBSERVATION: np.dtype(np.float32),
    episode_rewarder.ON_TARGET: np.dtype(np.float64),
    episode_rewarder.STOPPED: np.dtype(np.float64),
}


def postfix(tree, op_class, children, op_code):
    """(leaves in walk order, postfix list): an entry >= 0 is a leaf's number, a negative one an operation."""
    leaves, ops = [], []

    def walk(node):
        if isinstance(node, op_class):
            left, right = children(node)
            walk(left)
            walk(right)
            ops.append(op_code(node))
        else:
            assert not any(node is leaf for leaf in leaves), "a strategy object may occur only once in a composition"
            ops.append(len(leaves))
            leaves.append(node)

    walk(tree)
    return leaves, ops


def ender_postfix(ender):
    return postfix(ender, episode_ender.OpEnder, lambda node: (node._l_ender, node._r_ender),
                   lambda node: episode_ender.OR if node._op is np.bitwise_or else episode_ender.AND)


def rewarder_postfix(rewarder):
    return postfix(rewarder, episode_rewarder.OpRewarder, lambda node: (node._l_rewarder, node._r_rewarder),
                   lambda node: episode_rewarder.ADD if node._op is np.add else episode_rewarder.MUL)


def _number(x, what):
    assert isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool), f"{what}: {x!r} is not a number"
    assert math.isfinite(float(x)), f"{what}: {x!r} is not finite"
    return float(x)


def _state_index(i, what):
    assert isinstance(i, (int, np.integer)) and i in (0, 1), f"{what}: state index {i!r} outside {{0, 1}}"
    return int(i)


def _steps(k, what, most=2 ** 31 - 1):
    assert isinstance(k, (int, np.integer)) and 0 <= k <= most, f"{what}: {k!r} outside [0, {most}]"
    return int(k)


def _transformer(program, transformer, num_envs):
    assert isinstance(transformer, state_transformer.StateTransformer) and transformer.kind is not None, \
        f"unsupported transformer {transformer!r}"
    assert transformer.num_envs == num_envs, f"the transformer has num_envs {transformer.num_envs}, not {num_envs}"
    program.transformer = transformer.kind
    program.move_index = _state_index(transformer._move_index, "transformer move_index")
    assert len(transformer._limits) == 2, "transformer limits: (low, high)"
    program.limit_lo = _number(transformer._limits[0], "transformer limits")
    program.limit_hi = _number(transformer._limits[1], "transformer limits")
    if transformer.kind == state_transformer.CONTINUOUS_MOVE:
        program.speed = _number(transformer._speed, "ContinuousMoveTransformer speed")
    if transformer.kind in (state_transformer.CONTINUOUS_JUMP, state_transformer.CONTINUOUS_MOVE):
        program.stop_threshold = _number(transformer._stop_threshold, "transformer stop_threshold")
    else:
        action_set = transformer._action_set
        assert 1 <= len(action_set) <= 32, f"{len(action_set)} actions (1 to 32)"
        assert action_set.dtype.kind in "iuf", f"action set of dtype {action_set.dtype}"
        program.n_actions = len(action_set)
        for i, a in enumerate(action_set):
            program.action_set[i] = _number(a, "action set")


def _ender(leaf, num_envs):
    assert isinstance(leaf, episode_ender.BaseEnder) and leaf.kind is not None, f"unsupported ender {leaf!r}"
    assert leaf._num_envs == num_envs, f"{type(leaf).__name__} has num_envs {leaf._num_envs}, not {num_envs}"
    out = _native.EnvEnder()
    out.kind = leaf.kind
    name = type(leaf).__name__
    if leaf.kind in (episode_ender.DIVERGING, episode_ender.ON_TARGET):
        out.index0 = _state_index(leaf._check_indices[0], name)
        out.index1 = _state_index(leaf._check_indices[1], name)
        out.steps = _steps(leaf._early_end_steps, f"{name} early_end_steps")
        out.threshold = _number(leaf._threshold if leaf.kind == episode_ender.DIVERGING else leaf._radius, name)
    elif leaf.kind == episode_ender.STOPPED:
        out.index0 = _state_index(leaf._check_index, name)
        out.steps = _steps(leaf._early_end_steps, f"{name} early_end_steps", _native.MAX_STOPPED_STEPS)
        out.threshold = _number(leaf._early_end_span, name)
    elif leaf.kind == episode_ender.TIME_LIMIT:
        out.steps = _steps(leaf._max_steps, f"{name} max_steps")
    return out


def _rewarder(leaf, obs_width=4):
    assert isinstance(leaf, episode_rewarder.BaseRewarder) and leaf.kind is not None, f"unsupported rewarder {leaf!r}"
    name = type(leaf).__name__
    assert np.issubdtype(leaf.dtype, np.floating), f"{name}: numpy evaluates it in {leaf.dtype}, not floating point"
    assert leaf.dtype == LEAF_DTYPES[leaf.kind], \
        f"{name}: numpy evaluates it in {leaf.dtype}, the device in {LEAF_DTYPES[leaf.kind]} (Python-number or numpy.float64 parameters)"
    out = _native.EnvRewarder()
    out.kind = leaf.kind
    if leaf.kind == episode_rewarder.OBSERVATION:
        i = leaf._reward_observation_index
        assert isinstance(i, (int, np.integer)) and 0 <= i < obs_width, \
            f"{name}: observation index {i!r} outside 0-{obs_width - 1}"
        out.index0 = int(i)
        return out
    if leaf.kind in (episode_rewarder.DELTA, episode_rewarder.STOPPED):
        out.index0 = _state_index(leaf._check_index, name)
    else:
        out.index0 = _state_index(leaf._check_indices[0], name)
        out.index1 = _state_index(leaf._check_indices[1], name)
    params = {
        episode_rewarder.DELTA: lambda: (leaf._reward, leaf._scale, 0.0),
        episode_rewarder.DISTANCE: lambda: (leaf._span, leaf._width, leaf._low),
        episode_rewarder.ON_TARGET: lambda: (leaf._span, leaf._delta, leaf._off),
        episode_rewarder.STOPPED: lambda: (leaf._threshold, leaf._reward, 0.0),
    }[leaf.kind]()
    for k, value in enumerate(params):
        out.p[k] = _number(value, name)
    return out


def observer_nodes(observer):
    """The nodes of an observer tree in evaluation order: children before their wrapper, left to right.  A strategy
    object may occur only once."""
    nodes = []

    def walk(node):
        assert not any(node is other for other in nodes), "a strategy object may occur only once in a composition"
        for child in getattr(node, "_observers", ()):
            walk(child)
        nodes.append(node)

    walk(observer)
    return nodes


def _is_focus(node):
    return isinstance(node, state_observer.FocusObserver) or getattr(node, "kind", None) == state_observer.FOCUS


def focus_observer(observer):
    """The one FocusObserver of an observer tree: the environment renders with its renderer at its frame height.  None or
    several are refused: a step renders once (two would advance the RNG streams twice, none would be a step without a
    render, which is a different schedule)."""
    found = [node for node in observer_nodes(observer) if _is_focus(node)]
    assert len(found) == 1, f"{len(found)} FocusObservers in the observer tree (exactly one)"
    return found[0]


def compile_observer(observer, num_envs):
    """The rf_env_observer_program of an observer tree (AssertionError for anything the device cannot run).

    The nodes work on a stack of float32 columns per environment: an IndexedElementObserver or the FocusObserver writes
    the next free column; a DeltaObserver / NormalizedObserver works in place on the columns its children left, which are
    the top `width` ones, starting at `first` -- a DeltaObserver's changes replace them, or with include_original follow
    them.  The stack never shrinks, so the root's width is the most columns in use at any point."""
    nodes = observer_nodes(observer)
    focus_observer(observer)
    # (hstack(..., dtype=float32) is the wrappers'; the device's observations are float32 always)
    assert not _is_focus(observer), \
        "a FocusObserver alone observes in float64: wrap it (NormalizedObserver, DeltaObserver)"
    assert len(nodes) <= _native.MAX_OBS_NODES, f"{len(nodes)} observer nodes (at most {_native.MAX_OBS_NODES})"
    program = _native.EnvObserverProgram()
    program.n_nodes = len(nodes)
    starts = {}  # id(node) -> the first column of what it left
    top = n_old = 0
    for k, node in enumerate(nodes):
        name = type(node).__name__
        assert isinstance(node, state_observer.BaseObserver) and node.kind is not None, f"unsupported observer {node!r}"
        assert node.observation_space.shape[0] == num_envs, \
            f"{name} has num_envs {node.observation_space.shape[0]}, not {num_envs}"
        out = program.nodes[k]
        out.kind = node.kind
        if node.kind in (state_observer.INDEXED_ELEMENT, state_observer.FOCUS):
            assert node.single_observation_space.shape == (1,), f"{name}: not a scalar observer"
            if node.kind == state_observer.FOCUS:
                indices = (node._target_index, node._focus_plane_index)
                assert indices == (0, 1), f"{name}: (target_index, focus_plane_index) {indices!r} is not (0, 1)"
            else:
                out.index = _state_index(node._element_index, name)
            out.first, out.width = top, 1
            starts[id(node)] = top
            top += 1
        else:
            children = node._observers
            assert len(children) >= 1, f"{name}: no wrapped observers"
            out.first = starts[id(children[0])]
            out.width = top - out.first
            starts[id(node)] = out.first
            if node.kind == state_observer.DELTA:
                out.include_original = int(bool(node._include_original))
                out.old_first = n_old
                n_old += out.width
                top += out.width if node._include_original else 0
            else:
                bounds = np.concatenate([np.ravel(getattr(child.single_observation_space, b)) for child in children
                                         for b in ("low", "high")])
                # (the kernels clip with fminf / fmaxf, which do not propagate NaN as numpy.clip does)
                assert np.all(np.isfinite(bounds)), f"{name}: a wrapped bound is not finite"
                assert np.all(np.isfinite(node._mid)) and np.all(np.isfinite(node._scale)) and np.all(node._scale != 0), \
                    f"{name}: a scale is zero or not finite"
                for j in range(out.width):
                    out.mid[j] = float(node._mid[j])
                    out.scale[j] = float(node._scale[j])
        assert top <= _native.MAX_OBS_COLUMNS, f"{top} observation columns (at most {_native.MAX_OBS_COLUMNS})"
        assert n_old <= _native.MAX_OBS_COLUMNS, f"{n_old} delta old-value columns (at most {_native.MAX_OBS_COLUMNS})"
        assert node.single_observation_space.shape == (top - starts[id(node)],), f"{name}: its space is not what it observes"
    program.width = top
    program.n_old = n_old
    return program


def host_observer_state(observer, num_envs):
    """The DeltaObservers' old values of the host twin's tree, laid out as rf_env_get_observer_state returns them:
    float32[n_old, n], node-major in evaluation order."""
    rows = [node._old_wrapped_observations.T for node in observer_nodes(observer) if getattr(node, "kind", None) == state_observer.DELTA]
    return np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, num_envs), dtype=np.float32)


def compile_program(transformer, ender, rewarder, num_envs, observer=None):
    """The rf_env_program of a composition (AssertionError for anything the device cannot run); with an observer
    tree, (rf_env_program, rf_env_observer_program): an ObservationRewarder's index is then checked against that
    program's width in place of the built-in observer's four columns."""
    observer_program = None if observer is None else compile_observer(observer, num_envs)
    obs_width = 4 if observer is None else observer_program.width
    program = _native.EnvProgram()
    _transformer(program, transformer, num_envs)
    enders, ender_ops = ender_postfix(ender)
    assert len(enders) <= _native.MAX_LEAVES, f"{len(enders)} ender leaves (at most {_native.MAX_LEAVES})"
    program.n_enders = len(enders)
    program.n_ender_ops = len(ender_ops)
    for i, leaf in enumerate(enders):
        program.enders[i] = _ender(leaf, num_envs)
    for t, op in enumerate(ender_ops):
        program.ender_ops[t] = op
    rewarders, reward_ops = rewarder_postfix(rewarder)
    assert len(rewarders) <= _native.MAX_LEAVES, f"{len(rewarders)} rewarder leaves (at most {_native.MAX_LEAVES})"
    program.n_rewarders = len(rewarders)
    program.n_reward_ops = len(reward_ops)
    for i, leaf in enumerate(rewarders):
        program.rewarders[i] = _rewarder(leaf, obs_width)
    dtypes = []
    for t, op in enumerate(reward_ops):
        program.reward_ops[t] = op
        if op >= 0:
            dtypes.append(rewarders[op].dtype)
        else:
            right, left = dtypes.pop(), dtypes.pop()
            dtypes.append(np.promote_types(left, right))
        program.reward_f64[t] = int(dtypes[-1] == np.float64)
    return program if observer is None else (program, observer_program)


def compile_initializer(initializer):
    """The rf_env_initializer_program of a RangedInitializer over the two state elements (rf_env_configure_initializer):
    its ranges as float64 low / high - low, and its generator's state and increment as it stands now (the object itself
    is not advanced).  Every check of the library is made here first (AssertionError)."""
    assert isinstance(initializer, state_initializer.RangedInitializer), f"unsupported initializer {initializer!r}"
    ranges = initializer._ranges
    assert len(ranges) == 2, f"the initializer has {len(ranges)} elements, not the state's two"
    program = _native.EnvInitializerProgram()
    for j, element in enumerate(ranges):
        assert 1 <= len(element) <= _native.MAX_RANGES, f"element {j} has {len(element)} ranges (1 to {_native.MAX_RANGES})"
        program.counts[j] = len(element)
        for c, (low, high) in enumerate(element):
            low, high = _number(low, f"element {j} range {c}"), _number(high, f"element {j} range {c}")
            assert abs(low) < scalars.FLOAT32_BOUND and abs(high) < scalars.FLOAT32_BOUND, \
                f"element {j} range {c}: ({low!r}, {high!r}) is outside the float32 range"
            program.low[j][c] = low
            program.span[j][c] = float(initializer._highs[j][c] - initializer._lows[j][c])
            assert math.isfinite(program.span[j][c]) and abs(low + program.span[j][c]) < scalars.FLOAT32_BOUND, \
                f"element {j} range {c}: ({low!r}, {high!r}) is outside the float32 range"
    state, inc = initializer_state(initializer)
    program.state[0], program.state[1] = _native.words128(state)
    program.inc[0], program.inc[1] = _native.words128(inc)
    return program


def initializer_state(initializer):
    """(state, inc) of an initializer's numpy PCG64DXSM generator as Python ints."""
    state = initializer._generator.bit_generator.state
    assert state["bit_generator"] == "PCG64DXSM", f"the initializer draws from a {state['bit_generator']} generator"
    assert state["state"]["inc"] & 1, "the generator's increment is even"
    return state["state"]["state"], state["state"]["inc"]


def host_strategy_state(ender, rewarder, num_envs):
    """The per-leaf strategy state of the host twin's objects, laid out as rf_env_get_strategy_state returns it:
    (counters int32[n_enders, n], floats float32[n_enders, n], histories float32[rows, n], old float32[n_rewarders, n])."""
    enders, _ = ender_postfix(ender)
    rewarders, _ = rewarder_postfix(rewarder)
    counters = np.zeros((len(enders), num_envs), dtype=np.int32)
    floats = np.zeros((len(enders), num_envs), dtype=np.float32)
    histories = []
    for i, leaf in enumerate(enders):
        if leaf.kind == episode_ender.DIVERGING:
            counters[i] = leaf._diverging_steps
            floats[i] = leaf._last_diff
        elif leaf.kind == episode_ender.ON_TARGET:
            counters[i] = leaf._on_target_steps
        elif leaf.kind == episode_ender.TIME_LIMIT:
            counters[i] = leaf._steps
        elif leaf.kind == episode_ender.STOPPED:
            histories.append(leaf._moves.data.T)
    old = np.zeros((len(rewarders), num_envs), dtype=np.float32)
    for i, leaf in enumerate(rewarders):
        if leaf.kind in (episode_rewarder.DELTA, episode_rewarder.STOPPED) and leaf._old_states is not None:
            old[i] = leaf._old_states
    rows = np.concatenate(histories).astype(np.float32) if histories else np.zeros((0, num_envs), dtype=np.float32)
    return counters, floats, rows, old


def device_status(ender, state, index):
    """ender.status(index) of a composed environment from its device-side strategy state (rf_env_get_strategy_state):
    the status strings of the reference, leaf by leaf, joined as OpEnder joins them."""
    counters, _, histories, _ = state
    enders, _ = ender_postfix(ender)
    first_rows, row = [], 0
    for leaf in enders:
        first_rows.append(row)
        row += leaf._early_end_steps + 1 if leaf.kind == episode_ender.STOPPED else 0

    def walk(node):
        if isinstance(node, episode_ender.OpEnder):
            left, right = walk(node._l_ender), walk(node._r_ender)
            return left + (", " if left and right else "") + right
        i = next(k for k, leaf in enumerate(enders) if leaf is node)
        count = counters[i, index]
        if node.kind == episode_ender.DIVERGING:
            return f"diverging {count} / {node._early_end_steps}" if count > 0 else ""
        if node.kind == episode_ender.ON_TARGET:
            return f"on target {count} / {node._early_end_steps}" if count > 0 else ""
        if node.kind == episode_ender.TIME_LIMIT:
            return f"step {count} / {node._max_steps}"
        if node.kind == episode_ender.STOPPED:
            moves = histories[first_rows[i]:first_rows[i] + node._early_end_steps + 1, index]
            return episode_ender.stopped_status(moves, node._early_end_steps, node._early_end_span)
        return ""

    return walk(ender)
