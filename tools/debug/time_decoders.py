"""Diagnostic: times expand_kernel, wire_expand_kernel (decode on store) and record_gather_kernel on a C4 state
(128 envs, 40 scripted ticks) with the library NMMO_LIB names; one JSON line."""
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from nmmo_amd import abi
from nmmo_amd.config import Config
from nmmo_amd.engine import NmmoEngine
from nmmo_amd.storage import DeviceExperience

N, REPS = 128, 30
cfgs = {k: Config.preset("C4", MAP_N=16, early_stop_agent_num=8, obs_layout=lay)
        for k, lay in (("native", abi.OBS_NATIVE), ("wire", abi.OBS_WIRE), ("flat", abi.OBS_FLAT))}
engs = {k: NmmoEngine(c, N, seed=5) for k, c in cfgs.items()}
for e in engs.values():
    e.reset()
for t in range(40):
    for e in engs.values():
        e.scripted_actions(100 + t)
        e.step()
torch.cuda.synchronize()
flat, nat, wir = engs["flat"], engs["native"], engs["wire"]
P, elems, dev = flat.P, flat.obs_elems, flat.device
out = torch.empty((N, P, elems), dtype=torch.float32, device=dev)
z = torch.zeros(N * P, device=dev)
acts = torch.zeros((N * P, 12), dtype=torch.int32, device=dev)
m = flat.mask.reshape(-1).to(torch.uint8)
xw = DeviceExperience(N * P, elems, N * P, device=dev)
xr = DeviceExperience(N * P, elems, N * P, device=dev, record_arena_bytes=64 << 20)
xr.store(wir.obs, z, z.to(torch.uint8), m, acts, z, z, step=0, engine=wir)
k = xr.ptr
idx = torch.arange(k, dtype=torch.int32, device=dev)
got = torch.empty((k, elems), dtype=torch.float32, device=dev)

def timed(fn, pre=None):
    ts = []
    for i in range(REPS + 5):
        if pre:
            pre()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        if i >= 5:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}

res = {"lib": os.environ.get("NMMO_LIB", "tree"), "envs": N, "rows_in_realm": int(k), "reps": REPS}
res["expand_obs(native) [expand_kernel]"] = timed(lambda: nat.expand_obs(out=out))
res["store(wire, decode on store) [wire_expand_kernel + store]"] = timed(
    lambda: xw.store(wir.obs, z, z.to(torch.uint8), m, acts, z, z, step=0, engine=wir), pre=xw.reset)
res["gather_obs(records) [record_gather_kernel]"] = timed(lambda: xr.gather_obs(idx))
assert xw.ptr == k and xw.status == 0 and xr.status == 0
g = xr.gather_obs(idx)
assert torch.equal(g.view(torch.int32), xw.obs[:k].view(torch.int32))
res["sha_rows"] = __import__("hashlib").sha256(g.cpu().numpy().tobytes()).hexdigest()[:16]
res["sha_expand"] = __import__("hashlib").sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
print(json.dumps(res))
