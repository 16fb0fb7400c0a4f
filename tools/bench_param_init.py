"""Development benchmark of the parameter initialisation (include/reinfocus_hip.h, "parameter init"): one
init_parameters() call of a device population, both schemes, at two shapes --
  tuned      examples/ppo_tuned.yml's network: D = 25, pi = vf = [256, 256] (DevicePopulationPolicy);
  recurrent  sb3-contrib's recurrent defaults: D = 25, H = 256, pi = vf = [64, 64] (DevicePopulationLstmPolicy) --
for G = 1, 16, 64, 512:
  (a) population.init_parameters(seeds, ortho_init): two launches whatever G is (one for ortho_init=False at `tuned`);
  (b) what a user does without it: a Python loop over G constructions of the torch modules (nn.Linear / nn.LSTM with
      their default initialisation; torch.nn.init.orthogonal_ with SB3's gains and zero biases for the orthogonal scheme),
      their tensors moved to the device, and load_state_dict(group=g).
Alternating windows in one process, each a run of calls ended by one synchronisation; medians and the windows' spread.
No speed-up is promised: both sides are recorded.  One JSON line; --markdown FILE also rewrites the measured section of that
file (profiles/param_init.md), between its two marker lines.
usage (GPU box):  python tools/bench_param_init.py [--windows 5] [--groups 1,16,64,512] [--markdown profiles/param_init.md]"""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(HERE)
ARGV = list(sys.argv[1:])
from reinfocus_amd.environments import harness  # noqa: E402
from reinfocus_amd.environments import param_init  # noqa: E402

WIDTH = 25
BEGIN, END = "<!-- bench_param_init: begin -->", "<!-- bench_param_init: end -->"
SHAPES = {"tuned": dict(pi=(256, 256), vf=(256, 256)), "recurrent": dict(lstm_hidden=256, pi=(64, 64), vf=(64, 64))}


def option(name, default, kind=int):
    return kind(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def torch_state(spec, ortho_init):
    """One learner's state_dict as eager torch makes it: the modules' own initialisation, on the host, then to the device."""
    state, linear = {}, None
    for name, _, shape, is_weight in spec.entries:
        if name.endswith("weight_ih_l0"):
            lstm = torch.nn.LSTM(spec.obs_width, spec.lstm_hidden)
            prefix = name[:-len("weight_ih_l0")]
            for part in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                state[prefix + part] = getattr(lstm, part).detach()
        elif name.startswith(("lstm_actor.", "lstm_critic.")):
            continue
        elif name.endswith(".weight"):
            linear = torch.nn.Linear(shape[0], shape[1])
            if ortho_init and not name.startswith("critic."):
                gain = param_init.GAIN_EXTRACTOR if name.startswith("mlp_extractor.") else \
                    param_init.GAIN_ACTION if name.startswith("action_net.") else param_init.GAIN_VALUE
                torch.nn.init.orthogonal_(linear.weight, gain=gain)
                linear.bias.data.fill_(0.0)
            state[name] = linear.weight.detach()
        else:
            state[name] = linear.bias.detach()
    return {name: tensor.cuda() for name, tensor in state.items()}


def windows_of(forms, windows):
    """Microseconds per call: `windows` alternating windows per form, each `calls` calls of it and one synchronisation."""
    for form, _ in forms.values():  # warm-up
        form()
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, (form, calls) in forms.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(calls):
                form()
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - start) / calls)
    return {name: {"median_us": float(np.median(t)), "spread": float((max(t) - min(t)) / np.median(t)),
                   "windows_us": [round(x, 2) for x in t]} for name, t in times.items()}


def stage_times(shape, groups, windows):
    env = harness.DeviceVectorDiscreteSteps(num_envs=groups, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True)
    try:
        actions = int(env.single_action_space.n)
        if shape == "tuned":
            spec = harness.MlpPolicySpec(WIDTH, actions, **SHAPES[shape])
            many = harness.DevicePopulationPolicy(env, spec, groups, list(range(groups)))
        else:
            spec = harness.LstmPolicySpec(WIDTH, actions, **SHAPES[shape])
            many = harness.DevicePopulationLstmPolicy(env, spec, groups, list(range(groups)))
        seeds = list(range(100, 100 + groups))
        out = {"shape": shape, "groups": groups, "parameters": spec.size}
        for ortho_init in (False, True):
            def loop():
                for g in range(groups):
                    many.load_state_dict(torch_state(spec, ortho_init), group=g)

            out["ortho" if ortho_init else "uniform"] = windows_of(
                {"device": (lambda: many.init_parameters(seeds, ortho_init), max(3, 64 // groups)),
                 "loop": (loop, max(1, 8 // groups))}, windows)
        return out
    finally:
        env.close()


def markdown(stages):
    lines = [BEGIN, "", "| shape | G | scheme | init_parameters (us) | spread | loop over G torch constructions (us) | spread | "
             "loop / init_parameters |", "|---|---|---|---|---|---|---|---|"]
    for r in stages:
        for scheme in ("uniform", "ortho"):
            a, b = r[scheme]["device"], r[scheme]["loop"]
            lines.append(f"| {r['shape']} | {r['groups']} | {scheme} | {a['median_us']:.1f} | {100 * a['spread']:.0f} % | "
                         f"{b['median_us']:.1f} | {100 * b['spread']:.0f} % | {b['median_us'] / a['median_us']:.1f} |")
    return "\n".join(lines + ["", END])


def main():
    windows = option("--windows", 5)
    groups = [int(g) for g in option("--groups", "1,16,64,512", str).split(",")]
    torch.zeros(1, device="cuda")
    stages = []
    for shape in SHAPES:
        for g in groups:
            stages.append(stage_times(shape, g, windows))
            print(f"{shape}, G = {g}: measured", file=sys.stderr, flush=True)
    print(json.dumps({"windows": windows, "stages": stages}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(stages) + text[end:])


if __name__ == "__main__":
    main()
