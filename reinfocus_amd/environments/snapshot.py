"""Snapshots of the device-resident vector environments (harness.DeviceVectorDiscreteSteps, DeviceVectorContinuousJumps,
DeviceVectorEnvironment): what `env.snapshot()` returns and `env.restore()` takes.

An EnvSnapshot holds the library's blob (rf_env_snapshot, include/reinfocus_hip.h: states, counters, old values, scene
sets, the initializer's generator when it lives on the device, every pixel's RNG state) and, for an environment that
draws its reset states on the host, that generator's `bit_generator.state`.  Class name and constructor shape are kept
for error messages only: whether a blob fits an environment is the library's decision (the blob's fingerprint).

On disk a snapshot is one uncompressed .npz: the blob as a uint8 array and the small metadata as JSON text.  No pickle,
neither written nor read.
"""

import json

import numpy as np

FORMAT = 1
_KEYS = {"blob", "meta"}
_META = {"format", "env_class", "num_envs", "frame_height", "samples_per_pixel", "host_generator"}
_OPTIONAL = {"episode_records"}  # true when the environment keeps episode records; absent otherwise


def generator_to_json(state):
    """A numpy `bit_generator.state` dict as JSON-able values (the 128-bit words as hex text); None stays None."""
    if state is None:
        return None
    words = state["state"]
    assert set(words) == {"state", "inc"}, f"not the state of a PCG64 family generator: {sorted(words)}"
    return {"bit_generator": state["bit_generator"], "state": hex(words["state"]), "inc": hex(words["inc"]),
            "has_uint32": int(state["has_uint32"]), "uinteger": int(state["uinteger"])}


def generator_from_json(value):
    if value is None:
        return None
    return {"bit_generator": str(value["bit_generator"]),
            "state": {"state": int(value["state"], 16), "inc": int(value["inc"], 16)},
            "has_uint32": int(value["has_uint32"]), "uinteger": int(value["uinteger"])}


class EnvSnapshot:
    """blob: uint8[rf_env_snapshot_size]; host_generator: the host initializer's bit_generator.state, or None when the
    environment draws its reset states on the device (the generator is in the blob then)."""

    def __init__(self, blob, env_class, num_envs, frame_height, samples_per_pixel, host_generator=None,
                 episode_records=False):
        blob = np.asarray(blob)
        assert blob.dtype == np.uint8 and blob.ndim == 1, f"the blob is uint8[bytes], not {blob.dtype}{blob.shape}"
        self.blob = blob
        self.env_class = str(env_class)
        self.num_envs = int(num_envs)
        self.frame_height = int(frame_height)
        self.samples_per_pixel = int(samples_per_pixel)
        self.host_generator = host_generator
        self.episode_records = bool(episode_records)  # (the blob holds the episode accumulators)

    def describe(self):
        return (f"{self.env_class}(num_envs={self.num_envs}, frame_height={self.frame_height}, "
                f"samples_per_pixel={self.samples_per_pixel}, episode_records={self.episode_records})")

    def _meta(self):
        meta = {"format": FORMAT, "env_class": self.env_class, "num_envs": self.num_envs,
                "frame_height": self.frame_height, "samples_per_pixel": self.samples_per_pixel,
                "host_generator": generator_to_json(self.host_generator)}
        if self.episode_records:  # (left out when off: such a file is what it was before the flag existed)
            meta["episode_records"] = True
        return meta

    def save(self, path):
        """Writes the snapshot to `path` (exactly that name; no suffix is added)."""
        with open(path, "wb") as file:
            np.savez(file, blob=self.blob, meta=np.array(json.dumps(self._meta(), sort_keys=True)))

    @classmethod
    def load(cls, path):
        """Reads what save() wrote.  ValueError for a file that is not a snapshot: no blob, keys that do not belong,
        metadata that is not the expected JSON."""
        with np.load(path, allow_pickle=False) as data:
            keys = set(data.files)
            if keys != _KEYS:
                raise ValueError(f"{path}: not an environment snapshot (arrays {sorted(keys)}, expected {sorted(_KEYS)})")
            blob, meta = data["blob"], data["meta"]
        if blob.dtype != np.uint8 or blob.ndim != 1:
            raise ValueError(f"{path}: the blob is {blob.dtype}{blob.shape}, not uint8[bytes]")
        if meta.dtype.kind != "U" or meta.ndim != 0:
            raise ValueError(f"{path}: the metadata is {meta.dtype}{meta.shape}, not one JSON text")
        try:
            meta = json.loads(str(meta))
        except json.JSONDecodeError as error:
            raise ValueError(f"{path}: the metadata is not JSON ({error})") from None
        if not isinstance(meta, dict) or set(meta) - _OPTIONAL != _META:
            raise ValueError(f"{path}: metadata {sorted(meta) if isinstance(meta, dict) else type(meta).__name__}, "
                             f"expected {sorted(_META)}")
        if meta["format"] != FORMAT:
            raise ValueError(f"{path}: snapshot file format {meta['format']!r}, this package reads {FORMAT}")
        try:
            generator = generator_from_json(meta["host_generator"])
        except (KeyError, TypeError, ValueError) as error:
            raise ValueError(f"{path}: the host generator's state is malformed ({error!r})") from None
        if meta.get("episode_records", True) is not True:
            raise ValueError(f"{path}: episode_records is {meta['episode_records']!r}, not true or absent")
        return cls(blob, meta["env_class"], meta["num_envs"], meta["frame_height"], meta["samples_per_pixel"], generator,
                   "episode_records" in meta)
