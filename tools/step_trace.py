#!/usr/bin/env python
"""Call trace of the fused step's programs (cvhip/engine.py), for comparing schedules across commits.

For every configuration it builds the engine's programs for one batch size (nothing is launched) and prints,
per program key of `eng.graphs[n]` in a fixed order, the list of [name, lane, normalised args] of its calls and
the segment layout of the step.  It uses only ClearStep.build, _programs, _segments and Program.calls, so the
same file runs on any commit that has them.

Arguments are normalised so the trace does not depend on allocation addresses: Python ints below 2^16 and
c_float values print as their value, c_uint64 as "u64", None as itself, byref(struct) as "S:<type>", ctypes arrays
as "A:<type>x<len>", and any other integer (a device or host pointer, or a large size) as "p<k>" with k its index of
first appearance in that configuration's trace, which keeps aliasing visible.

    python tools/step_trace.py                 # every configuration, one JSON object, one line per configuration:
                                               # per program "<calls> <sha256 of its call list, 16 hex digits>"
    python tools/step_trace.py --full          # the call lists themselves (to diff two commits' schedules)
    python tools/step_trace.py --list          # the configuration names
    python tools/step_trace.py NAME [NAME...]  # only these (a data-parallel one must be the only one: it
                                               # initialises a world-1 process group, CVHIP_FORCE_DP=1)

tests/step_traces.json is this tool's default output; tests/test_gpu_step_trace.py regenerates it."""

import ctypes
import hashlib
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ("fwd", "fwd_g", "fwd_inj", "dec", "lat", "lat_inj", "enc", "enc2", "upd", "learn", "learn_inj", "dec_p",
        "enc_p", "upd_p", "pack_call")

# name -> (arch, z, n, mode, trainer options, engine module attributes)
BASE = {
    "c1_vae_clear_ps1": ("VAE", 16, 16, "clear", dict(ps=True), {}),
    "c2_vae_clear_ps0": ("VAE", 16, 16, "clear", dict(ps=False), {}),
    "c3_vae_clear_n512": ("VAE", 16, 512, "clear", dict(ps=True), {}),
    "c4_vae64_clear": ("VAE64", 64, 16, "clear", dict(ps=True), {}),
    "c5_vae64_mim_clubsample": ("VAE64", 64, 16, "mim", dict(est="CLUBSample"), {}),
    "c6_vae64_mim_club": ("VAE64", 64, 16, "mim", dict(est="CLUB"), {}),
    "c7_vae_tc": ("VAE", 16, 16, "tc", {}, {}),
    "c8_vae_group_mlvae": ("VAE", 16, 16, "group", dict(group="MLVAE"), {}),
    "c8_vae_group_gvae": ("VAE", 16, 16, "group", dict(group="GVAE"), {}),
    "c9_vae_clear_dp": ("VAE", 16, 16, "clear", dict(ps=True, dp=True), {}),
    "c9_vae_mim_dp": ("VAE", 16, 16, "mim", dict(est="CLUBSample", dp=True), {}),
}
# the kept schedule switches, each on configurations 1 and 4 (the MIM one on 5)
KNOBS = [("LATENT_AUX", False), ("LATENT_CHAIN", True), ("LATENT_AUX_OUT", True), ("LATENT_AUX_DL", 0),
         ("LATENT_AUX_DL", 2), ("DET_DZ", False), ("WGRAD_LANE", 0), ("WGRAD_LANE", 1), ("SPLIT_UPDATE", True),
         ("ADAM_PACK", "0"), ("ADAM_PACK", "1")]


def configs():
    out = dict(BASE)
    for knob, val in KNOBS:
        for base in ("c1_vae_clear_ps1", "c4_vae64_clear"):
            arch, z, n, mode, opts, _ = BASE[base]
            out[f"{base}+{knob}={int(val) if isinstance(val, bool) else val}"] = (arch, z, n, mode, opts, {knob: val})
    arch, z, n, mode, opts, _ = BASE["c1_vae_clear_ps1"]
    out["c1_vae_clear_ps1+SPLIT_UPDATE=1+ADAM_PACK=1"] = (arch, z, n, mode, opts,
                                                         {"SPLIT_UPDATE": True, "ADAM_PACK": "1"})
    arch, z, n, mode, opts, _ = BASE["c5_vae64_mim_clubsample"]
    for val in (0, 3):
        out[f"c5_vae64_mim_clubsample+MIM_BRANCHES={val}"] = (arch, z, n, mode, opts, {"MIM_BRANCHES": val})
    return out


def _trainer(arch, z, mode, opts):
    from src.utils import trainer_utils as T

    kw = dict(vae_arch=arch, in_channel=1 if arch == "VAE" else 3, device="cuda")
    if mode == "clear":
        return T.get_clearvae_trainer(beta=1 / 8, ps=opts["ps"], vae_lr=5e-4, z_dim=z, alpha=100, temperature=0.1, **kw)
    if mode == "mim":
        return T.get_clearmimvae_trainer(beta=1 / 8, mi_estimator=opts["est"], la=3.0, vae_lr=5e-4,
                                         mi_estimator_lr=2e-3, z_dim=z, alpha=100, temperature=0.1, **kw)
    if mode == "tc":
        return T.get_cleartcvae_trainer(beta=1 / 8, la=3.0, vae_lr=5e-4, factor_cls_lr=1e-3, z_dim=z, alpha=100,
                                        temperature=0.1, **kw)
    return T.get_hierarchical_vae_trainer(beta=1 / 8, vae_lr=5e-4, z_dim=z, group_mode=opts["group"], **kw)


class _Norm:
    """Argument normalisation of one configuration's trace (the pointer numbering is per configuration)."""

    def __init__(self):
        self.ptrs = {}

    def _ptr(self, v):
        return "p%d" % self.ptrs.setdefault(int(v), len(self.ptrs))

    def arg(self, a):
        import torch

        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, int):
            return a if 0 <= a < (1 << 16) else self._ptr(a)
        if isinstance(a, float):
            return a
        if isinstance(a, ctypes.c_float):
            return a.value
        if isinstance(a, ctypes.c_uint64):
            return "u64"
        if isinstance(a, ctypes.Array):
            return "A:%sx%d" % (a._type_.__name__, len(a))
        if isinstance(a, ctypes._Pointer):
            return self._ptr(ctypes.cast(a, ctypes.c_void_p).value or 0)
        if isinstance(a, torch.Tensor):
            return self._ptr(a.data_ptr())
        obj = getattr(a, "_obj", None)  # byref(struct)
        if isinstance(obj, ctypes.Structure):
            return "S:%s" % type(obj).__name__
        if isinstance(a, (list, tuple)):
            return [self.arg(v) for v in a]
        return "?:%s" % type(a).__name__

    def calls(self, calls):
        return [[name, lane, [self.arg(a) for a in args]] for name, _fn, args, lane in calls]


def trace(name):
    """The trace of one configuration: {"programs": {key: calls | {"same_as": key} | [[grad, adam], ...] | None},
    "segments": [...]}."""
    import torch

    from cvhip import engine
    from cvhip.engine import ClearStep

    arch, z, n, mode, opts, knobs = configs()[name]
    if opts.get("dp"):
        import torch.distributed as dist

        assert os.environ.get("CVHIP_FORCE_DP") == "1", "a data-parallel trace runs in its own process (main)"
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    prev = {k: getattr(engine, k) for k in knobs}
    try:
        for k, v in knobs.items():
            setattr(engine, k, v)
        eng = ClearStep.build(_trainer(arch, z, mode, opts), mode)
        assert eng is not None, name
        assert eng.dp == bool(opts.get("dp"))
        G = eng._programs(n)
        segs = eng._segments(G, False)
    finally:
        for k, v in prev.items():
            setattr(engine, k, v)
    norm = _Norm()
    seen = {}  # id(Program) -> first key
    progs = {}

    def one(key, P):
        if id(P) in seen:
            return {"same_as": seen[id(P)]}
        seen[id(P)] = key
        return norm.calls(P.calls)

    for key in KEYS:
        P = G.get(key)
        if P is None:
            progs[key] = None
        elif key == "pack_call":
            progs[key] = norm.calls([P])
        elif isinstance(P, list):  # data parallel: (gradient program, Adam program) per estimator update
            progs[key] = [[one(f"{key}[{j}].grad", gp), one(f"{key}[{j}].adam", ap)] for j, (gp, ap) in enumerate(P)]
        else:
            progs[key] = one(key, P)
    layout = []
    for item in segs:
        if item[0] == "prog":
            layout.append(["prog", [seen.get(id(P), "?") for P in item[1]]])
        else:
            layout.append(list(item))
    if opts.get("dp"):
        import torch.distributed as dist

        dist.destroy_process_group()
    return {"programs": progs, "segments": layout}


def trace_dp_child(name, timeout=120):
    """A data-parallel configuration in a fresh process (its own world-1 process group), under a time limit."""
    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, CVHIP_FORCE_DP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--full", name], env=env, capture_output=True,
                       text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}")
    head = json.dumps(name) + ": "  # (its own line of dumps(): anything else the process printed is skipped)
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith(head))
    return json.loads(line[len(head):].rstrip(","))


def digest(tr):
    """A trace with every call list replaced by "<number of calls> <sha256 of its compact JSON, 16 hex digits>": the
    committed form (the pointer numbering runs over the whole configuration, so aliasing between programs counts)."""
    def one(v):
        if v is None:
            return None
        if isinstance(v, dict):
            return "=" + v["same_as"]
        if v and isinstance(v[0][0], (list, dict)):  # data parallel: [[gradient program, Adam program], ...]
            return [[one(gp), one(ap)] for gp, ap in v]
        return "%d %s" % (len(v), hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).hexdigest()[:16])

    return {"programs": {k: one(v) for k, v in tr["programs"].items()}, "segments": tr["segments"]}


def dumps(traces):
    """One line per configuration (a readable diff), keys in configuration order."""
    body = ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in traces.items())
    return "{\n" + body + "\n}\n"


def main(argv):
    cfg = configs()
    if argv == ["--list"]:
        print("\n".join(cfg))
        return
    full = "--full" in argv
    names = [a for a in argv if a != "--full"] or list(cfg)
    in_child = os.environ.get("CVHIP_FORCE_DP") == "1"
    out = {}
    for name in names:
        if cfg[name][4].get("dp") and not in_child:
            out[name] = trace_dp_child(name)
        else:
            out[name] = trace(name)
    sys.stdout.write(dumps(out if full else {k: digest(v) for k, v in out.items()}))


if __name__ == "__main__":
    main(sys.argv[1:])
