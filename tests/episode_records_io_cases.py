"""TEST INFRASTRUCTURE: the child process of tests/test_gpu_episode_records.py's device-io tests.

As tests/device_io_cases.py: everything that needs torch and the library together runs in one fresh process that
imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.episode_records_io_cases <results.jsonl>
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("final_observation", "episode_return", "episode_length")
KINDS = ("composed-i64", "composed-i32", "jumps-f32")  # (tests/device_io_cases.py: TimeLimitEnder(3) | DivergingEnder)
N = 65


def _same_info(got, want, torch):
    """A step_tensors info against a host-form info, bit for bit (NaN equal to NaN)."""
    assert sorted(got) == sorted(KEYS) == sorted(want)
    dtypes = {"final_observation": torch.float32, "episode_return": torch.float64, "episode_length": torch.int32}
    for key in KEYS:
        assert got[key].dtype == dtypes[key] and got[key].device.type == "cuda", key
        x, y = got[key].cpu().numpy(), want[key]
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), key


def mixed_case(torch, cases, kind):
    """step_tensors and step() mixed step by step on one context against a twin context stepped through step()."""
    twin = cases.make_env(kind, N, episode_records=True)
    dev = cases.make_env(kind, N, episode_records=True)
    twin.reset()
    _, info = dev.reset_tensors()
    assert info == {}
    rng = np.random.default_rng(6)
    ended, owned = [], None
    for step in range(12):
        actions = cases.host_actions(kind, rng, N)
        want = twin.step(actions)
        if step % 3 == 1:  # the host form in between
            got = dev.step(actions)
            assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4]))
            for key in KEYS:
                assert np.array_equal(got[4][key], want[4][key], equal_nan=True), key
        else:
            got = dev.step_tensors(torch.from_numpy(actions).cuda())
            for x, y in zip(got[:4], want[:4]):
                assert np.array_equal(x.cpu().numpy(), y)
            _same_info(got[4], want[4], torch)
            pointers = [got[4][key].data_ptr() for key in KEYS]  # (owned by the environment: one set)
            assert owned is None or owned == pointers
            owned = pointers
        for x, y in zip(dev.episode_accumulators(), twin.episode_accumulators()):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        ended.append(int(want[3].sum()))
    # (the task's own ender ends all environments at once; the composition's ends a part of them in every step)
    assert any(0 < k < N for k in ended) if kind.startswith("composed") else sum(ended) > 0, ended
    assert dev.device_fault() is None
    twin.close()
    dev.close()


def out_case(torch, cases):
    """out= keeps its three-tuple meaning: the caller's tensors are filled, the records stay the environment's."""
    kind = "composed-i64"
    twin = cases.make_env(kind, N, episode_records=True)
    dev = cases.make_env(kind, N, episode_records=True)
    twin.reset()
    dev.reset_tensors()
    out = (torch.full((N, 4), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((N,), 7.0, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"))
    rng = np.random.default_rng(3)
    for _ in range(4):
        actions = cases.host_actions(kind, rng, N)
        want = twin.step(actions)
        got = dev.step_tensors(torch.from_numpy(actions).cuda(), out=out)
        assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
        assert np.array_equal(out[2].cpu().numpy().astype(bool), want[3])
        _same_info(got[4], want[4], torch)
    twin.close()
    dev.close()


def queue_case(torch, cases):
    """6 steps enqueued back to back, nothing read in between: each step's info tensors are cloned on torch's stream,
    and every clone equals the host-form run made afterwards."""
    kind = "composed-i32"
    twin = cases.make_env(kind, N, episode_records=True)
    dev = cases.make_env(kind, N, episode_records=True)
    dev.reset_tensors()
    rng = np.random.default_rng(9)
    taken = [cases.host_actions(kind, rng, N) for _ in range(6)]
    staged = [torch.from_numpy(a).cuda() for a in taken]
    torch.cuda.synchronize()
    kept = []
    for actions in staged:
        info = dev.step_tensors(actions)[4]
        kept.append({key: info[key].clone() for key in KEYS})
    torch.cuda.synchronize()
    twin.reset()
    ended = []
    for actions, clone in zip(taken, kept):
        want = twin.step(actions)
        _same_info(clone, want[4], torch)
        ended.append(int(want[3].sum()))
    assert any(0 < k < N for k in ended), ended
    twin.close()
    dev.close()


def refusal_case(torch, cases):
    """Record pointers on a records-off context, and a record pointer that is host memory: RF_ERR_INVALID, nothing
    changes."""
    kind = "composed-i32"
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    obs = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    rewards = torch.empty(N, dtype=torch.float64, device="cuda")
    flags = torch.empty(N, dtype=torch.uint8, device="cuda")
    final = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    returns = torch.empty(N, dtype=torch.float64, device="cuda")
    lengths = torch.empty(N, dtype=torch.int32, device="cuda")

    def refused(call, match):
        try:
            call()
        except AssertionError as caught:
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")

    def records_step(env, final_ptr, returns_ptr, lengths_ptr):
        env._ctx.env_step_device_records(actions.data_ptr(), 0, obs.data_ptr(), rewards.data_ptr(), flags.data_ptr(), None,
                                         final_ptr, returns_ptr, lengths_ptr, 0)

    for records in (False, True):
        dev = cases.make_env(kind, N, episode_records=records)
        twin = cases.make_env(kind, N, episode_records=records)
        dev.reset_tensors()
        twin.reset()
        before = cases.everything(dev)
        if records:
            host_array = np.zeros(N, dtype=np.float64)
            refused(lambda: records_step(dev, final.data_ptr(), host_array.ctypes.data, lengths.data_ptr()),
                    "d_returns is not device memory")
            host_rows = np.zeros((N, 4), dtype=np.float32)
            refused(lambda: records_step(dev, host_rows.ctypes.data, None, None), "d_final_obs is not device memory")
        else:
            for pointers in ((final.data_ptr(), None, None), (None, returns.data_ptr(), None),
                             (None, None, lengths.data_ptr())):
                refused(lambda: records_step(dev, *pointers), "keeps no episode records")
            records_step(dev, None, None, None)  # (three NULLs: rf_env_step_device itself)
            want = twin.step(np.zeros(N, dtype=np.int32))
            assert np.array_equal(obs.cpu().numpy(), want[0])
            before = cases.everything(dev)
        after = cases.everything(dev)
        assert before[1] == after[1] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[0], after[0]))
        want = twin.step(np.zeros(N, dtype=np.int32))
        got = dev.step_tensors(actions)  # ... and the environment still steps
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and sorted(got[4]) == sorted(want[4])
        dev.close()
        twin.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    for kind in KINDS:
        with record.case(f"mixed/{kind}"):
            mixed_case(torch, cases, kind)
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
