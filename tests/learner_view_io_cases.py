"""TEST INFRASTRUCTURE: the child process of tests/test_gpu_learner_view.py's device-io tests.

As tests/episode_records_io_cases.py: everything that needs torch and the library together runs in one fresh process
that imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.learner_view_io_cases <results.jsonl>
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STACK = 65, 5


def _bits(a):
    return a.dtype.str, a.shape, a.tobytes()


def _view():
    from reinfocus_amd.environments import harness

    return harness.LearnerView(frame_stack=STACK)


def _same_step(got, want, torch, tensors):
    """A step's five results against a host-form step's, as bytes; tensors: `got` is step_tensors'."""
    assert sorted(got[4]) == sorted(want[4])
    pairs = list(zip(got[:4], want[:4])) + [(got[4][key], want[4][key]) for key in sorted(want[4])]
    for index, (x, y) in enumerate(pairs):
        if tensors:
            assert isinstance(x, torch.Tensor) and x.device.type == "cuda", index
            x = x.cpu().numpy()
        assert _bits(x) == _bits(np.asarray(y)), f"result {index} differs"


def _same_view(dev, twin):
    for x, y in zip(dev.view_state(), twin.view_state()):
        assert _bits(x) == _bits(y)
    a, b = dev.view_statistics(), twin.view_statistics()
    assert all(_bits(a[key]) == _bits(b[key]) for key in ("mean", "var", "count"))


def mixed_case(torch, cases, kind, records):
    """step_tensors and step() mixed step by step on one context against a twin context stepped through step()."""
    twin = cases.make_env(kind, N, episode_records=records, learner_view=_view())
    dev = cases.make_env(kind, N, episode_records=records, learner_view=_view())
    want_obs, want_info = twin.reset()
    obs, info = dev.reset_tensors()
    assert sorted(info) == ["raw_observation"] and obs.shape == (N, 4 * STACK) and obs.dtype == torch.float32
    assert _bits(obs.cpu().numpy()) == _bits(want_obs)
    assert _bits(info["raw_observation"].cpu().numpy()) == _bits(want_info["raw_observation"])
    _same_view(dev, twin)
    rng = np.random.default_rng(6)
    ended, owned = [], None
    for step in range(12):
        actions = cases.host_actions(kind, rng, N)
        want = twin.step(actions)
        if step % 3 == 1:  # the host form in between
            _same_step(dev.step(actions), want, torch, False)
        else:
            got = dev.step_tensors(torch.from_numpy(actions).cuda())
            _same_step(got, want, torch, True)
            pointers = [got[0].data_ptr(), got[1].data_ptr()] + [got[4][key].data_ptr() for key in sorted(got[4])]
            assert owned is None or owned == pointers  # (owned by the environment: one set)
            owned = pointers
        _same_view(dev, twin)
        ended.append(int(want[3].sum()))
    assert any(0 < k < N for k in ended) if kind.startswith("composed") else sum(ended) > 0, ended
    assert dev.device_fault() is None
    twin.close()
    dev.close()


def out_case(torch, cases):
    """out= means the view's observation and reward; the raw ones stay the environment's."""
    kind = "composed-i64"
    twin = cases.make_env(kind, N, episode_records=True, learner_view=_view())
    dev = cases.make_env(kind, N, episode_records=True, learner_view=_view())
    twin.reset()
    dev.reset_tensors()
    out = (torch.full((N, 4 * STACK), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((N,), 7.0, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"))
    rng = np.random.default_rng(3)
    for _ in range(4):
        actions = cases.host_actions(kind, rng, N)
        want = twin.step(actions)
        got = dev.step_tensors(torch.from_numpy(actions).cuda(), out=out)
        assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
        _same_step(got, want, torch, True)
        assert np.array_equal(out[2].cpu().numpy().astype(bool), want[3])
    try:
        dev.step_tensors(torch.from_numpy(actions).cuda(), out=(torch.empty((N, 4), dtype=torch.float32, device="cuda"),
                                                                 out[1], out[2]))
    except ValueError as caught:
        assert "shape" in str(caught)
    else:
        raise AssertionError("a raw-shaped out[0] was taken")
    twin.close()
    dev.close()


def queue_case(torch, cases):
    """6 steps enqueued back to back, nothing read in between: each step's results are cloned on torch's stream, and
    every clone equals the host-form run made afterwards."""
    kind = "composed-i32"
    twin = cases.make_env(kind, N, episode_records=True, learner_view=_view())
    dev = cases.make_env(kind, N, episode_records=True, learner_view=_view())
    dev.reset_tensors()
    rng = np.random.default_rng(9)
    taken = [cases.host_actions(kind, rng, N) for _ in range(6)]
    staged = [torch.from_numpy(a).cuda() for a in taken]
    torch.cuda.synchronize()
    kept = []
    for actions in staged:
        got = dev.step_tensors(actions)
        kept.append(tuple(x.clone() for x in got[:4]) + ({key: value.clone() for key, value in got[4].items()},))
    torch.cuda.synchronize()
    twin.reset()
    for actions, clone in zip(taken, kept):
        _same_step(clone, twin.step(actions), torch, True)
    _same_view(dev, twin)
    twin.close()
    dev.close()


def refusal_case(torch, cases):
    """View pointers on a context without a view, d_view_final without records, a view pointer that is host memory:
    RF_ERR_INVALID, nothing changes."""
    kind = "composed-i32"
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    obs = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    rewards = torch.empty(N, dtype=torch.float64, device="cuda")
    flags = torch.empty(N, dtype=torch.uint8, device="cuda")
    view_obs = torch.empty((N, 4 * STACK), dtype=torch.float32, device="cuda")
    view_final = torch.empty((N, 4 * STACK), dtype=torch.float32, device="cuda")
    view_rewards = torch.empty(N, dtype=torch.float64, device="cuda")

    def refused(call, match):
        try:
            call()
        except AssertionError as caught:
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")

    def view_step(env, obs_ptr, rewards_ptr, final_ptr):
        env._ctx.env_step_device_view(actions.data_ptr(), 0, obs.data_ptr(), rewards.data_ptr(), flags.data_ptr(), None,
                                      None, None, None, obs_ptr, rewards_ptr, final_ptr, 0)

    plain = cases.make_env(kind, N)
    plain.reset_tensors()
    before = cases.everything(plain)
    for pointers in ((view_obs.data_ptr(), None, None), (None, view_rewards.data_ptr(), None)):
        refused(lambda: view_step(plain, *pointers), "no learner view")
    refused(lambda: plain._ctx.env_reset_device_view(obs.data_ptr(), view_obs.data_ptr(), 0), "no learner view")
    after = cases.everything(plain)
    assert before[1] == after[1] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[0], after[0]))
    plain.close()

    dev = cases.make_env(kind, N, learner_view=_view())  # (no records)
    twin = cases.make_env(kind, N, learner_view=_view())
    dev.reset_tensors()
    twin.reset()
    before, state = cases.everything(dev), dev.view_state()
    refused(lambda: view_step(dev, view_obs.data_ptr(), view_rewards.data_ptr(), view_final.data_ptr()),
            "needs episode records")
    host_rows = np.zeros((N, 4 * STACK), dtype=np.float32)
    refused(lambda: view_step(dev, host_rows.ctypes.data, None, None), "d_view_obs is not device memory")
    host_rewards = np.zeros(N, dtype=np.float64)
    refused(lambda: view_step(dev, None, host_rewards.ctypes.data, None), "d_view_rewards is not device memory")
    after = cases.everything(dev)
    assert before[1] == after[1] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[0], after[0]))
    assert all(_bits(x) == _bits(y) for x, y in zip(state, dev.view_state()))
    want = twin.step(np.zeros(N, dtype=np.int32))
    _same_step(dev.step_tensors(actions), want, torch, True)  # ... and the environment still steps
    # the plain device forms keep the view going: its state advances although nobody takes the outputs
    want = twin.step(np.zeros(N, dtype=np.int32))
    dev._ctx.env_step_device(actions.data_ptr(), 0, obs.data_ptr(), rewards.data_ptr(), flags.data_ptr(), None, 0)
    assert _bits(obs.cpu().numpy()) == _bits(want[4]["raw_observation"])
    _same_view(dev, twin)
    dev.close()
    twin.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    for kind, records in (("composed-i64", True), ("composed-i32", False), ("jumps-f32", True)):
        with record.case(f"mixed/{kind}"):
            mixed_case(torch, cases, kind, records)
    with record.case("out"):
        out_case(torch, cases)
    with record.case("queue"):
        queue_case(torch, cases)
    with record.case("refusals"):
        refusal_case(torch, cases)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
