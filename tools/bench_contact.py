#!/usr/bin/env python3
"""Cost of penalty contact in an explicit step on the stretched, jittered Kuhn cube (prints one JSON line).

Mesh, material and load of tools/bench_explicit.py: mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2), Ti-6Al-4V,
linear material, here with the far face z = 2 clamped and the face z = 0 free. In one process, each a warm-up run and
then `--steps` steps at dt = 0.9 x the guaranteed stable step in ONE ExplicitDynamics.run between two device events:
  plain      no contact set (the step as it was before contact existed: the yardstick)
  untouched  a plane and a sphere attached (mu = 0.3), both out of reach of every node
  touching   the same two, the plane rising into the face z = 0 at 1 m/s from 1e-5 inside it: the whole face in contact
             at the first step, then thrown ahead and caught again (the counts at the first and last step come from
             one-step runs around the timed one), the sphere away
No history or energy rows in the timed runs: two launches per step in all three.

    python tools/bench_contact.py --cube-n 55 > profiles/contact_n55.json
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import mesh, system  # noqa: E402

E, NU, RHO = 113.8e9, 0.342, 4430.0
F64 = torch.float64


def run_case(coords, tets, mask, surfaces, steps, warmup):
    xd = system.ExplicitDynamics(coords, tets, RHO, E, NU, "linear", mask)
    try:
        dt = 0.9 * xd.stable_dt()[0]
        out = {"dt": dt, "steps": steps}
        if surfaces:
            xd.set_contact(surfaces, 0.5, dt=dt)
        xd.start()
        if surfaces:
            out["in_contact_first"] = xd.run(1, dt, contact_every=1).in_contact[0].tolist()
        xd.run(warmup, dt)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        res = xd.run(steps, dt)    # + one force evaluation for the state reached
        b.record()
        torch.cuda.synchronize()
        out["ms_per_step"] = a.elapsed_time(b) / (steps + 1)
        if surfaces:
            last = xd.run(1, dt, contact_every=1)
            out["in_contact_last"] = last.in_contact[0].tolist()
            out["penetration_last"] = last.penetration[0].tolist()
        out["status"], out["u_max"] = res.status, float(xd.u.abs().max())
        assert math.isfinite(out["u_max"]) and res.status == system.XD_OK
        return out
    finally:
        xd.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)
    N = coords.shape[0]
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[mesh.face_nodes(coords, 2, 2.0)] = 1
    mask = mask.view(-1)
    sphere = dict(kind="sphere", point=[0.5, 0.35, 5.0], radius=0.5, friction=0.3)
    far = [system.RigidSurface("plane", [0.0, 0.0, -1.0], normal=[0, 0, 1], friction=0.3), system.RigidSurface(**sphere)]
    near = [system.RigidSurface("plane", [0.0, 0.0, 1e-5], normal=[0, 0, 1], friction=0.3, velocity=[0.0, 0.0, 1.0]),
            system.RigidSurface(**sphere)]
    out = {"tool": "bench_contact", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "nodes": N,
           "face_nodes": int(mesh.face_nodes(coords, 2, 0.0).numel())}
    for name, surfaces in (("plain", None), ("untouched", far), ("touching", near)):
        out[name] = run_case(coords, tets, mask, surfaces, a.steps, a.warmup)
    for name in ("untouched", "touching"):
        out[name + "_over_plain"] = out[name]["ms_per_step"] / out["plain"]["ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
