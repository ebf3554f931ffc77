"""The reference's run_fall_test.sh, batched: B robots of one gait (model, pgs id), each kicked
differently (synth.gen_kicks), each stopped once fall_check (player.cpp:669-681) would have ended
its process. One hs_sim_trial launch instead of B runs of the binary; the tally is
hs_sim_trial_summary's.

  python tools/fall_test.py --rollouts 4096 --kick 0 100 --plane xy --hc 0.7 --steps 300 --bins 10
  python tools/fall_test.py --rollouts 4096 --steps 200 --no-kicks --no-check --time --vs-step

Prints the fallen / survived / running counts, the fall-time quantiles and (--bins) the fall
fraction per kick-magnitude bin, then one JSON line. --time measures the launch with HIP events
after --warmup steps, --repeats times (every repeat from the reset state; the median is reported), as
bench.py --sim does, and reports simulation steps/s counting only the steps actually taken;
--vs-step times hs_sim_step on the same batch the same way.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PGS_MODEL_DEFAULT = {"hexapod": 8, "spider": 24, "myant": 9}


def window(dt, tmin, tmax):
    """first tsi whose tsi * dt is not < tmin; last tsi whose tsi * dt is not > tmax (-1: no end)"""
    lo = 0
    if tmin > 0:
        lo = max(0, int(tmin / dt) - 2)
        while lo * dt < tmin:
            lo += 1
    if tmax is None or tmax / dt >= 2e9:
        return lo, -1
    hi = int(tmax / dt) + 2
    while hi > 0 and hi * dt > tmax:
        hi -= 1
    return lo, hi


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="hexapod", choices=sorted(PGS_MODEL_DEFAULT))
    ap.add_argument("--pgs", type=int, default=None, help="pgs_config.txt setup id (default: the model's)")
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--kick", type=float, nargs=2, default=(0.0, 100.0), metavar=("LO", "HI"),
                    help="kick magnitude range (velocity change)")
    ap.add_argument("--plane", default="xz", choices=("xz", "xy"))
    ap.add_argument("--kick-every", type=int, default=500)
    ap.add_argument("--kick-phase", type=int, default=None, help="default kick_every - 1 (player.cpp:589)")
    ap.add_argument("--no-kicks", action="store_true")
    ap.add_argument("--hc", type=float, default=0.7)
    ap.add_argument("--tmin", type=float, default=0.0)
    ap.add_argument("--tmax", type=float, default=None, help="default: no end")
    ap.add_argument("--no-check", action="store_true", help="fall check off (nothing freezes)")
    ap.add_argument("--torque-limit", type=float, default=0.0)
    ap.add_argument("--open-loop", action="store_true")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--tsi0", type=int, default=2)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--bins", type=int, default=0, help="fall fraction per kick-magnitude bin")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--vs-step", action="store_true", help="with --time: hs_sim_step on the same batch too")
    ap.add_argument("--occupancy", action="store_true",
                    help="print the resident rollouts per CU of the kernel's builds for the three models and exit")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch

    import hslabs_amd as H
    from hslabs_amd import synth

    if args.occupancy:
        import ctypes
        from hslabs_amd import capi

        torch.zeros(1, device="cuda")
        names = ("fp64", "fp64 trial", "fp32", "fp32 trial", "fp32 3w", "fp32 3w trial")
        for n, m_max, who in ((18, 144, "spider-size (18 parts, 144 rows)"), (22, 176, "hexapod-size (22, 176)"),
                              (24, 216, "largest (24, 216)")):
            o = (ctypes.c_int32 * 6)()
            assert capi.load().hs_debug_sim_occupancy(n, m_max, o) == 0
            print(f"{who}: " + ", ".join(f"{k} {v}" for k, v in zip(names, o)) + " rollouts per CU")
        return
    B = args.rollouts
    model = H.KinematicModel(os.path.join(ROOT, "models", f"{args.model}.xml"))
    pgs_id = PGS_MODEL_DEFAULT[args.model] if args.pgs is None else args.pgs
    p = H.read_pgs_config(os.path.join(ROOT, "models", "pgs_config.txt"), pgs_id)
    dtype = torch.float32 if args.fp32 else torch.float64
    sb = H.SimBatch(model, [p] * B, tsi0=args.tsi0, dtype=dtype)
    dt = sb.params.dt
    lo, hi = window(dt, args.tmin, args.tmax)
    kw = dict(open_loop=args.open_loop, torque_limit=args.torque_limit, hc=args.hc,
              check_from=(2 ** 31 - 1) if args.no_check else lo, check_until=-1 if args.no_check else hi)
    dv = None
    if not args.no_kicks:
        seed = {} if args.seed is None else dict(seed=args.seed)
        dv = synth.gen_kicks(B, args.kick[0], args.kick[1], plane=args.plane, **seed)
        kw.update(kick_every=args.kick_every, kick_phase=args.kick_phase,
                  kick_dv=torch.as_tensor(dv, dtype=dtype, device=sb.device))
    stream = torch.cuda.current_stream(sb.device)
    none = dict(tau_cmd=False)  # no per-step outputs

    def fresh():
        sb.reset(args.tsi0)
        sb.trial_reset()

    def timed(job):
        """median kernel ms over the repeats, each from the reset state after a warm-up launch"""
        ms = []
        for _ in range(args.repeats):
            fresh()
            if args.warmup:
                sb.step(args.warmup, stream=stream, outputs=())
                fresh()
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            job()
            ev1.record(stream)
            torch.cuda.synchronize()
            ms.append(ev0.elapsed_time(ev1))
        return float(np.median(ms)), ms

    out = {"model": args.model, "pgs": pgs_id, "rollouts": B, "steps": args.steps, "dtype": "f32" if args.fp32 else "f64",
           "hc": args.hc, "check_from": kw["check_from"], "check_until": kw["check_until"]}
    if args.time:
        ms, all_ms = timed(lambda: sb.trial(args.steps, stream=stream, **kw, **none))
        taken = int((sb.tsi.long() - args.tsi0).sum().item())
        out.update(kernel_ms=round(ms, 3), kernel_ms_all=[round(v, 3) for v in all_ms], steps_taken=taken,
                   steps_per_s=round(taken / (ms * 1e-3), 1))
        print(f"trial: {ms:.2f} ms per launch (median of {args.repeats}), {taken} steps taken of {B * args.steps}, "
              f"{taken / (ms * 1e-3) / 1e6:.3f} M steps/s")
        if args.vs_step:
            state = sb.state.clone()
            ms_s, all_s = timed(lambda: sb.step(args.steps, stream=stream, outputs=()))
            sb.state.copy_(state)
            out.update(step_kernel_ms=round(ms_s, 3), step_kernel_ms_all=[round(v, 3) for v in all_s],
                       step_steps_per_s=round(B * args.steps / (ms_s * 1e-3), 1),
                       trial_vs_step=round((taken / ms) / (B * args.steps / ms_s), 4))
            print(f"hs_sim_step: {ms_s:.2f} ms per launch, {B * args.steps / (ms_s * 1e-3) / 1e6:.3f} M steps/s; "
                  f"trial / step rate = {out['trial_vs_step']}")
    else:
        sb.trial(args.steps, stream=stream, **kw, **none)
        torch.cuda.synchronize()
    s = sb.trial_summary()
    out.update(s)
    print(f"fallen {s['fallen']}  survived {s['survived']}  running {s['running']}  of {B}")
    st = sb.state.cpu().numpy()
    fell = st >= 0
    if fell.any():
        q = np.quantile(st[fell] * dt, [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1])
        out["fall_t_quantiles"] = [round(float(v), 4) for v in q]
        print("fall time quantiles (min 10% 25% 50% 75% 90% max): " + " ".join(f"{v:.2f}" for v in q))
        assert s["min_fall_tsi"] == st[fell].min() and s["sum_fall_tsi"] == st[fell].astype(np.int64).sum()
    if args.bins and dv is not None:
        mag = np.linalg.norm(dv, axis=1)
        edges = np.linspace(args.kick[0], args.kick[1], args.bins + 1)
        idx = np.clip(np.digitize(mag, edges) - 1, 0, args.bins - 1)
        rows = []
        print("kick magnitude      rollouts  fallen  fraction")
        for i in range(args.bins):
            n, f = int((idx == i).sum()), int((fell & (idx == i)).sum())
            rows.append([round(float(edges[i]), 3), round(float(edges[i + 1]), 3), n, f])
            print(f"{edges[i]:7.1f} - {edges[i + 1]:7.1f}  {n:8d}  {f:6d}  {f / max(n, 1):8.3f}")
        out["bins"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
