#!/usr/bin/env python3
"""Time SimBatch.estimate_B (hs_sim_estimate_B: "dynamics from simulation").

Builds a batch of B robots, walks it a few steps so that the tracker has a history, then times
  estimate   one estimate_B call: configuration, tracker push, B * m probes, accelerations, regression;
  probe      the probe launch alone (hs_sim_probe);
  regress    the regression alone (hs_sim_regress_B on the estimate's T and U);
  baseline   (--baseline) what a caller could do for the probes before hs_sim_probe existed: copy every
             body state m times, build B * m one-row torque tables and run hs_sim_trial open-loop for one
             step on the B * m rollouts -- no configurations, accelerations or regression.
Device events around `--iters` back-to-back calls, after `--warmup` calls; `--reps` rounds alternate the
variants (interleaved A/B), medians are reported. One JSON line at the end.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="hexapod")
    ap.add_argument("--pgs", type=int, default=8, help="pgs_config.txt setup id")
    ap.add_argument("-B", type=int, default=256)
    ap.add_argument("-m", type=int, default=None, help="probes per rollout (default config_dim + 20)")
    ap.add_argument("--walk", type=int, default=25, help="steps taken before the timing")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()

    import torch

    import hslabs_amd as H
    from hslabs_amd import capi, synth

    if not torch.cuda.is_available():
        sys.exit("estimate_b.py needs a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = H.KinematicModel(os.path.join(root, "models", f"{a.model}.xml"))
    p = H.read_pgs_config(os.path.join(root, "models", "pgs_config.txt"), a.pgs)
    B, nmj, cfg = a.B, model.nmj, model.config_dim
    m = a.m if a.m is not None else cfg + 20
    sb = H.SimBatch(model, [p] * B)
    for _ in range(a.walk):
        sb.track_push()
        sb.step(1, outputs=("tau_cmd",))
    dev = sb.device
    dtau = torch.as_tensor(synth.gen_torque_perturbations(B, m, nmj), device=dev)
    tau0 = sb.last_tau.clone()
    state = (sb.seed.clone(), sb.ders.clone())

    def restore():
        sb.seed.copy_(state[0])
        sb.ders.copy_(state[1])

    est = sb.estimate_B(dtau=dtau, tau0=tau0)
    T, U = est["T"].clone(), est["U"].clone()
    rank_ok = bool((est["rank"] == nmj + 1).all())
    restore()

    variants = {"estimate": lambda: sb.estimate_B(dtau=dtau, tau0=tau0),
                "probe": lambda: sb.probe(dtau, tau0=tau0),
                "regress": lambda: sb.regress_B(T, U)}
    if a.baseline:
        L = capi.load()
        n = B * m
        rep_body = torch.empty((n, model.n_parts, capi.SIM_BODY_STRIDE), dtype=torch.float64, device=dev)
        rep_seed = torch.zeros(n, dtype=torch.int32, device=dev)
        rep_tsi = torch.zeros(n, dtype=torch.int32, device=dev)
        rep_state = torch.full((n,), capi.HS_TRIAL_RUNNING, dtype=torch.int32, device=dev)
        t = capi.SimTrialArgsC()
        s = t.sim
        s.n_rollouts, s.n_steps, s.n_t, s.precision = n, 1, 1, capi.HS_PREC_F64
        s.params = sb.params
        s.params.k = 0.0  # open loop applies the table row whatever k is; k = 0 needs no q / dq tables
        t.open_loop, t.check_from, t.check_until = 1, 10 ** 9, -1
        t.state = rep_state.data_ptr()

        def baseline():
            rep_body.view(B, m, -1).copy_(sb.body.view(B, 1, -1).expand(B, m, -1))
            rep_seed.view(B, m).copy_(sb.seed.view(B, 1).expand(B, m))
            rep_tsi.zero_()
            tab = tau0[:, None, :] + dtau
            s.body, s.seed, s.tsi = rep_body.data_ptr(), rep_seed.data_ptr(), rep_tsi.data_ptr()
            s.tau_tab = tab.data_ptr()
            s.stream = torch.cuda.current_stream(dev).cuda_stream
            capi.check(L.hs_sim_trial(model.handle, ctypes.byref(t)), "hs_sim_trial")
            return tab

        variants["baseline"] = baseline

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():  # alternating: one window of each per round
            ms[k].append(timed(fn))
            restore()
    res = {"tool": "estimate_b", "model": a.model, "B": B, "m": m, "iters": a.iters, "reps": a.reps,
           "rank_full": rank_ok, "lib": capi.LOADED}
    for k, v in ms.items():
        res[f"{k}_ms"] = round(statistics.median(v), 4)
        res[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        print(f"{k:9s} {statistics.median(v):9.4f} ms per call (min {min(v):.4f}, max {max(v):.4f})")
    res["probes_per_s"] = round(B * m / (res["probe_ms"] * 1e-3))
    res["estimate_probes_per_s"] = round(B * m / (res["estimate_ms"] * 1e-3))
    print(f"probes per second: {res['probes_per_s']:.4g} (probe launch), {res['estimate_probes_per_s']:.4g} "
          "(whole estimate)")
    if a.baseline:
        res["baseline_over_probe"] = round(res["baseline_ms"] / res["probe_ms"], 3)
        res["baseline_over_estimate"] = round(res["baseline_ms"] / res["estimate_ms"], 3)
        print(f"baseline / probe {res['baseline_over_probe']}, baseline / estimate {res['baseline_over_estimate']}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
