"""modelplayer::cpc_test (player.cpp:440-449), batched: B robots of one gait walk --walk steps under position
control with the B estimate running (the reference's first steps, player.cpp:468; at least 2, so that the tracker
has its pushes), then --steps steps of configuration path control on the estimated B (hs_sim_cpc_step), each
robot kicked differently (synth.gen_kicks) and stopped once fall_check (player.cpp:669-681) would have ended its
process, as tools/fall_test.py does for position control.

  python tools/cpc_test.py --rollouts 4096 --kick 0 100 --plane xy --hc 0.7 --steps 300 --bins 10 --vs-position
  python tools/cpc_test.py --rollouts 4096 --no-kicks --no-check --time

--vs-position runs the same kicks under hs_sim_trial's PD law from the same walked state and prints both fall
fractions by kick bin. --time prints device-event ms per CPC step (the whole hs_sim_cpc_step call) next to its
parts launched alone from the same state -- the estimate, the controller, one open-loop trial step -- and the
regression launch alone: medians and min / max over --rounds alternating rounds.
The probes' torque perturbations are drawn on the device from gen_torque_perturbations' distribution
(player.cpp:567: 100 levels in [-0.4, 0.4)), a fresh set per step, --chunk steps per call.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PGS_MODEL_DEFAULT = {"hexapod": 8, "spider": 24, "myant": 9}


def main():
    from fall_test import window

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="hexapod", choices=sorted(PGS_MODEL_DEFAULT))
    ap.add_argument("--pgs", type=int, default=None)
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--walk", type=int, default=2, help="position-control steps with estimates before CPC (>= 2)")
    ap.add_argument("--steps", type=int, default=300, help="CPC steps")
    ap.add_argument("--m", type=int, default=None, help="probes per estimate (default config_dim + 20)")
    ap.add_argument("--chunk", type=int, default=8, help="CPC steps per hs_sim_cpc_step call")
    ap.add_argument("--kick", type=float, nargs=2, default=(0.0, 100.0), metavar=("LO", "HI"))
    ap.add_argument("--plane", default="xz", choices=("xz", "xy"))
    ap.add_argument("--kick-every", type=int, default=500)
    ap.add_argument("--kick-phase", type=int, default=None)
    ap.add_argument("--no-kicks", action="store_true")
    ap.add_argument("--hc", type=float, default=0.7)
    ap.add_argument("--tmin", type=float, default=0.0)
    ap.add_argument("--tmax", type=float, default=None)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--torque-limit", type=float, default=0.0)
    ap.add_argument("--tsi0", type=int, default=2)
    ap.add_argument("--seed", type=int, default=None, help="kicks and perturbations (default: fall_test.py's kicks)")
    ap.add_argument("--bins", type=int, default=0)
    ap.add_argument("--vs-position", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4, help="with --time: calls per timed window")
    args = ap.parse_args()
    if args.walk < 2:
        ap.error("--walk must be at least 2: the tracker needs two pushes before its rates mean anything")

    import torch

    import hslabs_amd as H
    from hslabs_amd import synth

    if not torch.cuda.is_available():
        sys.exit("cpc_test.py needs a GPU")
    B = args.rollouts
    model = H.KinematicModel(os.path.join(ROOT, "models", f"{args.model}.xml"))
    pgs_id = PGS_MODEL_DEFAULT[args.model] if args.pgs is None else args.pgs
    p = H.read_pgs_config(os.path.join(ROOT, "models", "pgs_config.txt"), pgs_id)
    sb = H.SimBatch(model, [p] * B, tsi0=args.tsi0)
    dev, nmj, cfg = sb.device, model.nmj, model.config_dim
    m = cfg + 20 if args.m is None else args.m
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed or 0)

    def draw(n_steps):
        k = torch.randint(0, 100, (n_steps, B, m, nmj), device=dev, generator=gen)
        return ((k - 50).to(torch.float32).to(torch.float64) / 50.) * 0.4

    # the reference's first steps: estimate_B, then position control
    for _ in range(args.walk):
        sb.estimate_B(dtau=draw(1)[0])
        sb.step(1, outputs=("tau_cmd",))
    sb.cpc_target_points()
    torch.cuda.synchronize()
    walked = dict(body=sb.body.clone(), seed=sb.seed.clone(), tsi=sb.tsi.clone(), ders=sb.ders.clone(),
                  last_tau=sb.last_tau.clone())

    def restore():
        sb.body.copy_(walked["body"])
        sb.seed.copy_(walked["seed"])
        sb.tsi.copy_(walked["tsi"])
        sb.ders.copy_(walked["ders"])
        sb.last_tau = walked["last_tau"].clone()
        if getattr(sb, "low_tpdist", None) is not None:
            sb.low_tpdist.fill_(1)
            sb.last_tpi.zero_()
        sb.trial_reset()

    lo, hi = window(sb.params.dt, args.tmin, args.tmax)
    kw = dict(torque_limit=args.torque_limit, hc=args.hc, check_from=(2 ** 31 - 1) if args.no_check else lo,
              check_until=-1 if args.no_check else hi)
    dv = None
    if not args.no_kicks:
        dv = synth.gen_kicks(B, args.kick[0], args.kick[1], plane=args.plane,
                             **({} if args.seed is None else dict(seed=args.seed)))
        kw.update(kick_every=args.kick_every, kick_phase=args.kick_phase,
                  kick_dv=torch.as_tensor(dv, dtype=torch.float64, device=dev))
    out = {"tool": "cpc_test", "model": args.model, "pgs": pgs_id, "rollouts": B, "walk": args.walk, "steps": args.steps,
           "m": m, "hc": args.hc, "lib": H.capi.LOADED}

    def fall_table(tag, st):
        fell = st >= 0
        res = {"fallen": int(fell.sum()), "survived": int((st == H.capi.HS_TRIAL_SURVIVED).sum()),
               "running": int((st == H.capi.HS_TRIAL_RUNNING).sum())}
        print(f"{tag}: fallen {res['fallen']}  survived {res['survived']}  running {res['running']}  of {B}")
        if args.bins and dv is not None:
            mag = np.linalg.norm(dv, axis=1)
            edges = np.linspace(args.kick[0], args.kick[1], args.bins + 1)
            idx = np.clip(np.digitize(mag, edges) - 1, 0, args.bins - 1)
            res["bins"] = [[round(float(edges[i]), 3), round(float(edges[i + 1]), 3), int((idx == i).sum()),
                            int((fell & (idx == i)).sum())] for i in range(args.bins)]
        return res

    def run_cpc():
        restore()
        flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        done = 0
        while done < args.steps:
            n = min(args.chunk, args.steps - done)
            o = sb.cpc_step(n, dtau=draw(n), **kw)
            # a frozen rollout's tracker is pushed the same configuration again: its rates are 0, every loss is
            # 0 / 0 and the controller flags it; only the rollouts still walking are reported
            flags |= torch.where(sb.state == H.capi.HS_TRIAL_RUNNING, o["flags"], torch.zeros_like(flags))
            done += n
        torch.cuda.synchronize()
        return sb.state.cpu().numpy().copy(), flags.cpu().numpy()

    if args.time:
        restore()
        d1 = draw(1)[0].contiguous()
        dn = draw(args.chunk)
        est = sb.estimate_B(dtau=d1)
        Bt, T, U = est["Bt"].clone(), est["T"].clone(), est["U"].clone()
        ctl = sb.cpc_torques(Bt)
        tab = ctl["tau"].clone()
        L, capi = H.capi.load(), H.capi
        import ctypes

        t = capi.SimTrialArgsC()
        s = t.sim
        s.n_rollouts, s.n_steps, s.n_t, s.precision = B, 1, 1, capi.HS_PREC_F64
        s.params = sb.params
        s.params.k = 0.0
        t.open_loop, t.check_from, t.check_until = 1, 2 ** 31 - 1, -1
        state = torch.full((B,), capi.HS_TRIAL_RUNNING, dtype=torch.int32, device=dev)
        t.state = state.data_ptr()

        def trial_step():
            s.body, s.seed, s.tsi = sb.body.data_ptr(), sb.seed.data_ptr(), sb.tsi.data_ptr()
            s.tau_tab = tab.data_ptr()
            s.stream = torch.cuda.current_stream(dev).cuda_stream
            capi.check(L.hs_sim_trial(model.handle, ctypes.byref(t)), "hs_sim_trial")

        nokick = dict(check_from=2 ** 31 - 1)
        variants = {"cpc_step": (lambda: sb.cpc_step(args.chunk, dtau=dn, **nokick), args.chunk),
                    "estimate": (lambda: sb.estimate_B(dtau=d1), 1),
                    "controller": (lambda: sb.cpc_torques(Bt), 1),
                    "regress": (lambda: sb.regress_B(T, U), 1),
                    "trial_step": (trial_step, 1)}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters

        for fn, _ in variants.values():
            restore()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (fn, steps) in variants.items():  # alternating: one window of each per round
                restore()
                torch.cuda.synchronize()
                ms[k].append(timed(fn) / steps)
        for k, v in ms.items():
            out[f"{k}_ms"] = round(statistics.median(v), 4)
            out[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            print(f"{k:11s} {statistics.median(v):9.4f} ms per step (min {min(v):.4f}, max {max(v):.4f})")
        parts = out["estimate_ms"] + out["controller_ms"] + out["trial_step_ms"]
        out["parts_ms"] = round(parts, 4)
        out["controller_share"] = round(out["controller_ms"] / out["cpc_step_ms"], 4)
        out["controller_over_regress"] = round(out["controller_ms"] / out["regress_ms"], 3)
        print(f"cpc step {out['cpc_step_ms']:.4f} ms; estimate + controller + trial step launched alone {parts:.4f} ms; "
              f"controller share {out['controller_share']:.3f}; controller / regression {out['controller_over_regress']}")
    else:
        st, flags = run_cpc()
        out["cpc"] = fall_table("CPC", st)
        out["cpc_flags_seen_while_walking"] = int(np.bitwise_or.reduce(flags)) if len(flags) else 0
        out["finite"] = bool(torch.isfinite(sb.body).all().item())
        if args.vs_position:
            restore()
            sb.trial(args.steps, tau_cmd=False, **kw)
            torch.cuda.synchronize()
            out["position"] = fall_table("position control", sb.state.cpu().numpy())
            if "bins" in out["cpc"]:
                print("kick magnitude      rollouts  CPC fallen  fraction   PD fallen  fraction")
                for (a, b, n, f), (_, _, _, g) in zip(out["cpc"]["bins"], out["position"]["bins"]):
                    print(f"{a:7.1f} - {b:7.1f}  {n:8d}  {f:10d}  {f / max(n, 1):8.3f}  {g:10d}  {g / max(n, 1):8.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
