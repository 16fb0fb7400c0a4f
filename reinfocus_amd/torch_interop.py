"""torch tensors in, torch tensors out: the device-resident environments stepped from a policy network on the same GPU
without the actions, observations, rewards or flags ever crossing to the host, and without a host synchronisation
(rf_env_step_device, rf_env_reset_device; include/reinfocus_hip.h "device io").

torch is imported here and only here, and only when one of the *_tensors methods of an environment is called: the
package and the C ABI stay torch-free, and `import reinfocus_amd` does not import torch.

ONE HIP RUNTIME PER PROCESS.  torch's wheel carries its own libamdhip64.so with the same soname as the ROCm
installation's.  A stream handle or a device pointer means something only to the runtime that made it, so torch and
libreinfocus_hip.so must share one.  They do when torch is imported BEFORE the library is loaded -- the library's
dependency then resolves to the runtime that is mapped already.  `import reinfocus_amd` loads nothing (the library is
loaded by the first environment or renderer), so either import order works; what does not work is creating an
environment first and importing torch afterwards: torch then maps a second runtime next to the first.
check_one_runtime() counts the mappings and says so instead of letting handles of one runtime reach the other.
"""

import os

_one_runtime_checked = False


def _torch():
    import torch

    return torch


def hip_runtimes():
    """The distinct libamdhip64 files this process has mapped (/proc/self/maps)."""
    found = set()
    with open("/proc/self/maps") as maps:
        for line in maps:
            fields = line.split(None, 5)
            if len(fields) == 6 and os.path.basename(fields[5].strip()).startswith("libamdhip64"):
                found.add(os.path.realpath(fields[5].strip()))
    return sorted(found)


def check_one_runtime():
    """RuntimeError if torch and the library do not share one HIP runtime (checked once, after both are loaded)."""
    global _one_runtime_checked
    if _one_runtime_checked:
        return
    found = hip_runtimes()
    if len(found) > 1:
        raise RuntimeError(
            "this process has mapped %d HIP runtimes (%s): torch's streams and tensors mean nothing to the runtime "
            "libreinfocus_hip.so uses.  Import torch before the first reinfocus_amd environment or renderer is "
            "created (`import reinfocus_amd` itself loads nothing), so that the library binds to the runtime torch "
            "brought" % (len(found), ", ".join(found)))
    _one_runtime_checked = True


class TensorIO:
    """What an environment's reset_tensors / step_tensors / device_fault do, for one context (a _native.Context, or in
    tests anything with its env_*_device methods): `num_envs` environments with observations of `obs_width` columns on
    HIP device `device_index`; float_actions: the task takes torch.float32 actions, not torch.int32 / int64 indices."""

    def __init__(self, ctx, num_envs, obs_width, float_actions, device_index, episode_records=False, view_stack=0):
        """episode_records: the context keeps them (rf_env_configure_records) -- step() then goes through
        rf_env_step_device_records and its info holds the three record tensors, owned like the other outputs.
        view_stack: the frame_stack of the context's learner view (rf_env_configure_view; 0: none) -- step() then goes
        through rf_env_step_device_view: obs (float32 [n, view_stack * W]) and rewards are the view's -- out= means
        them --, info holds "raw_observation" and "raw_reward" (and with records the view's "final_observation" next to
        "raw_final_observation") as owned tensors, and reset_viewed() is the reset."""
        self._ctx = ctx
        self._records = bool(episode_records)
        self._owned_records = None
        self._view_stack = int(view_stack)
        self._owned_view = None
        self._n = int(num_envs)
        self._width = int(obs_width)
        self._float = bool(float_actions)
        self._index = int(device_index)
        self._owned = None

    # -- arguments, checked before the library is called ---------------------------------------------------------
    def checked_actions(self, actions):
        """The library's dtype code of `actions` (ACTION_I32 / _I64 / _F32); TypeError / ValueError for anything but a
        contiguous [n] or [n, 1] tensor of the task's dtype on the environment's GPU.  float64 is refused like any other
        dtype: the caller casts, so the rounding is theirs."""
        from reinfocus_amd import _native

        torch = _torch()
        if not isinstance(actions, torch.Tensor):
            raise TypeError(f"actions must be a torch.Tensor on cuda:{self._index}, not {type(actions).__name__}")
        codes = ({torch.float32: _native.ACTION_F32} if self._float
                 else {torch.int32: _native.ACTION_I32, torch.int64: _native.ACTION_I64})
        if actions.dtype not in codes:
            raise TypeError("actions are %s, but the task takes %s (cast them: the rounding is the caller's)"
                            % (actions.dtype, " or ".join(str(d) for d in codes)))
        if tuple(actions.shape) not in ((self._n,), (self._n, 1)):
            raise ValueError(f"actions have shape {tuple(actions.shape)}, not ({self._n},) or ({self._n}, 1)")
        if not actions.is_contiguous():
            raise ValueError("actions are not contiguous (strided tensors are not taken: call .contiguous())")
        self._on_device(actions, "actions")
        return codes[actions.dtype]

    def _on_device(self, tensor, what):
        if tensor.device.type != "cuda" or tensor.device.index != self._index:
            raise ValueError(f"{what} live on {tensor.device}, but the environment runs on cuda:{self._index}: "
                             "a device step reads and writes device memory of its own GPU only")

    def _checked_out(self, out):
        torch = _torch()
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise TypeError("out must be (obs, rewards, truncated)")
        wanted = (("out[0] (obs)", (torch.float32,), (self._n, self._width * max(self._view_stack, 1))),
                  ("out[1] (rewards)", (torch.float64,), (self._n,)),
                  ("out[2] (truncated)", (torch.bool, torch.uint8), (self._n,)))
        for tensor, (what, dtypes, shape) in zip(out, wanted):
            if not isinstance(tensor, torch.Tensor):
                raise TypeError(f"{what} must be a torch.Tensor, not {type(tensor).__name__}")
            if tensor.dtype not in dtypes:
                raise TypeError(f"{what} is {tensor.dtype}, not {' or '.join(str(d) for d in dtypes)}")
            if tuple(tensor.shape) != shape:
                raise ValueError(f"{what} has shape {tuple(tensor.shape)}, not {shape}")
            if not tensor.is_contiguous():
                raise ValueError(f"{what} is not contiguous")
            self._on_device(tensor, what)
        return tuple(out)

    # -- the environment's own tensors --------------------------------------------------------------------------
    def _outputs(self):
        """(obs, rewards, truncated uint8, terminated, count), made once: every call without out= overwrites them."""
        if self._owned is None:
            torch = _torch()
            device = torch.device("cuda", self._index)
            self._owned = (torch.empty((self._n, self._width), dtype=torch.float32, device=device),
                           torch.empty(self._n, dtype=torch.float64, device=device),
                           torch.zeros(self._n, dtype=torch.uint8, device=device),
                           torch.zeros(self._n, dtype=torch.bool, device=device),
                           torch.zeros(1, dtype=torch.int32, device=device))
        return self._owned

    def _record_outputs(self):
        """(final_observation float32 [n, W], episode_return float64 [n], episode_length int32 [n]), made once and
        overwritten by every step."""
        if self._owned_records is None:
            torch = _torch()
            device = torch.device("cuda", self._index)
            self._owned_records = (torch.empty((self._n, self._width), dtype=torch.float32, device=device),
                                   torch.empty(self._n, dtype=torch.float64, device=device),
                                   torch.empty(self._n, dtype=torch.int32, device=device))
        return self._owned_records

    def _view_outputs(self):
        """(view observation float32 [n, V], view reward float64 [n], view final_observation float32 [n, V] or None),
        made once and overwritten by every step without out=."""
        if self._owned_view is None:
            torch = _torch()
            device = torch.device("cuda", self._index)
            cells = self._width * self._view_stack
            self._owned_view = (torch.empty((self._n, cells), dtype=torch.float32, device=device),
                                torch.empty(self._n, dtype=torch.float64, device=device),
                                torch.empty((self._n, cells), dtype=torch.float32, device=device) if self._records
                                else None)
        return self._owned_view

    def _stream(self):
        torch = _torch()
        return torch.cuda.current_stream(torch.device("cuda", self._index)).cuda_stream

    # -- the calls -------------------------------------------------------------------------------------------------
    def reset(self):
        _torch()
        check_one_runtime()
        obs = self._outputs()[0]
        self._ctx.env_reset_device(obs.data_ptr(), self._stream())
        return obs

    def reset_viewed(self):
        """reset() of a context with a learner view: (view observation, {"raw_observation": obs}), both owned."""
        _torch()
        check_one_runtime()
        raw, view = self._outputs()[0], self._view_outputs()[0]
        self._ctx.env_reset_device_view(raw.data_ptr(), view.data_ptr(), self._stream())
        return view, {"raw_observation": raw}

    def _step_viewed(self, actions, code, out):
        torch = _torch()
        owned, (view_obs, view_rewards, view_final) = self._outputs(), self._view_outputs()
        truncated = owned[2]
        if out is not None:
            view_obs, view_rewards, truncated = self._checked_out(out)
        info = {"raw_observation": owned[0], "raw_reward": owned[1]}
        record_ptrs = (None, None, None)
        if self._records:
            final_obs, returns, lengths = self._record_outputs()
            record_ptrs = (final_obs.data_ptr(), returns.data_ptr(), lengths.data_ptr())
            info.update(final_observation=view_final, raw_final_observation=final_obs, episode_return=returns,
                        episode_length=lengths)
        self._ctx.env_step_device_view(actions.data_ptr(), code, owned[0].data_ptr(), owned[1].data_ptr(),
                                       truncated.data_ptr(), owned[4].data_ptr(), *record_ptrs, view_obs.data_ptr(),
                                       view_rewards.data_ptr(), None if view_final is None else view_final.data_ptr(),
                                       self._stream())
        flags = truncated if truncated.dtype == torch.bool else truncated.view(torch.bool)
        return view_obs, view_rewards, owned[3], flags, info

    def step(self, actions, out=None):
        code = self.checked_actions(actions)
        check_one_runtime()
        if self._view_stack:
            return self._step_viewed(actions, code, out)
        torch = _torch()
        owned = self._outputs()
        obs, rewards, truncated = owned[:3] if out is None else self._checked_out(out)
        info = {}
        if self._records:
            final_obs, returns, lengths = self._record_outputs()
            self._ctx.env_step_device_records(actions.data_ptr(), code, obs.data_ptr(), rewards.data_ptr(),
                                              truncated.data_ptr(), owned[4].data_ptr(), final_obs.data_ptr(),
                                              returns.data_ptr(), lengths.data_ptr(), self._stream())
            info = {"final_observation": final_obs, "episode_return": returns, "episode_length": lengths}
        else:
            self._ctx.env_step_device(actions.data_ptr(), code, obs.data_ptr(), rewards.data_ptr(), truncated.data_ptr(),
                                      owned[4].data_ptr(), self._stream())
        flags = truncated if truncated.dtype == torch.bool else truncated.view(torch.bool)
        return obs, rewards, owned[3], flags, info

    def fault(self):
        """The synchronising query: None, or (step, env) of the earliest invalid action since the last reset."""
        return self._ctx.env_device_status()

    def reset_count(self):
        """How many environments ended in the last device step (synchronises)."""
        self._ctx.env_device_status()
        return int(self._outputs()[4].item())
