"""Probe (not a test): launch extents of the C4 batch's LM passes against the scenes really active, and what the two kernels
with the most expensive empty workgroups (k_schur_f, k_eval) cost per launch and per live scene.

  run:   python tools/probes/probe_pass_extents.py run [scenes]        (under rocprofv3 --kernel-trace --stats --output-format csv;
         one scene group, one warm solve, then one solve with PTZ_BA_DEBUG_TIMING=2, whose per-pass lines go to stderr.
         Fill the scene cache in a plain process first: under the tracer the generator's forked pool workers do not exit,
         profiles/NOTES_r08.md section 4)
  join:  python tools/probes/probe_pass_extents.py join <stderr-file> <dir-with-kernel_trace.csv>
         -> one line per pass (shape, slots, host count, live scenes, k_schur_f us, k_eval us) and the sums per ladder shape"""
import csv, glob, os, re, sys

if sys.argv[1] == "run":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    os.environ["PTZ_BA_STREAMS"] = "1"
    scenes = pkg.synth.make_scenes(range(n), 200, 500, cache_dir=os.environ.get("PTZ_SCENE_CACHE", "/tmp/ptz_scene_cache"))
    b = pkg.api.BaBatch(scenes); b.set_state(); b.solve()
    os.environ["PTZ_BA_DEBUG_TIMING"] = "2"
    b.set_state(); s = b.solve()
    print("lm_steps", sum(x["num_lm_steps"] for x in s), "device ms", round(b.last_solve_ms(), 2))
else:
    passes = [tuple(int(v) for v in m.groups()) for m in
              re.finditer(r"pass g(\d+) p(\d+): shape (\d+), (\d+) slots, host count (\d+), live (\d+)", open(sys.argv[2]).read())]
    f = sorted(glob.glob(os.path.join(sys.argv[3], "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))
    us = {}
    for key in ("k_schur_f", "k_eval<"):
        d = [(e - s) / 1e3 for s, e, name in rows if key in name]
        us[key] = d[-len(passes):]  # the launches of the last solve, in pass order
    print("pass shape slots host_count live schur_us eval_us")
    tot = {}
    for (g, p, si, slots, cnt, live), a, e in zip(passes, us["k_schur_f"], us["k_eval<"]):
        print(p, si, slots, cnt, live, round(a, 1), round(e, 1))
        t = tot.setdefault(si, [0, 0, 0, 0.0, 0.0]); t[0] += 1; t[1] += slots; t[2] += live; t[3] += a; t[4] += e
    print("shape passes slots live empty schur_ms eval_ms schur_us_per_live eval_us_per_live")
    for si, (k, slots, live, a, e) in sorted(tot.items()):
        print(si, k, slots, live, slots - live, round(a / 1e3, 2), round(e / 1e3, 2), round(a / max(live, 1), 2), round(e / max(live, 1), 2))
