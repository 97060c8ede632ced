"""Device time of the posterior map summary (slamgpu_map_summary: map_summary_kernel + map_finish_kernel), in one process:

  (a) example_webmap, 10^5 particles, known association (compact genealogy), after 100 observation steps;
  (b) config 5 (FastSLAM 2, 10^5 particles, the synthetic 10^4-landmark map, slot capacity 10^4, plain rows, log-weights) after 200
      steps of slamgpu_run_particle through the candidate lists.

Each figure: the kernels' time between event pairs on the context's stream (slamgpu_profile / slamgpu_kernel_time: every chunk's two
launches), and the whole call between two events (launches + the copies of the result, ending in a synchronisation); 2 calls of
warm-up, the median of 7.  Algorithmic bytes: 24 B per (particle, slot) + the weight once per particle and group of 8 slots.

    python tools/map_summary_probe.py [--out profiles/map_summary.txt]

--trace JSON: config 5 driven by the host (slamgpu_update_particle through the grid, census every step: pp_holders_kernel counts the
partial slots' holders through the same genealogy), 220 steps, a summary before each of the last 120 -- for a run under
rocprofv3 --kernel-trace --stats; the slots the census visited are written to JSON.
--summarize STATS_CSV JSON: time per (particle, slot) visited of pp_holders_kernel and of map_summary_kernel from that run.
--pairs: the joint shares (slamgpu_map_pairs: map_pairs_kernel + map_finish_kernel) on the same two states: on (a) all pairs a < b of the
slots in use, on (b) all pairs of slots whose posterior means lie within 1 m (slamhost_map_candidates); kernel time and call time as above,
beside slamgpu_map_summary on the same state in the same process per (particle, record) read, and algorithmic bytes (2 x (4 + 20) B per
particle and pair: two genealogy entries, two records) over the kernel time; then what slamhost_map_merge makes of them (radius 1 m,
cohold 0.1).  --tape: config 5's whole tape (2 172 steps, run_particle through the lists, exclusion rule with the spacing cap f = 0.5, slot capacity
15 000, log-weights: tools/particle_excl_spacing_probe.py's arm), then the posterior map beside the best particle's."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slam_amd  # noqa: E402
from particle_lists_probe import OPT, EXCL_OFF, EXCL_ON, config5_map, context, course, device_steps, host_steps  # noqa: E402

N = 100000
PEAK = 8.0e12       # B/s, HBM3E
COPY = (4.9e12, 5.3e12)  # the copy rate README.md records for this part


def bytes_of(n, slots):
    return 24.0 * n * slots + 4.0 * n * ((slots + 7) // 8)


def timed_summaries(s, calls=7, warm=2):
    """(kernel ms, whole-call ms) of `calls` summaries over all slots after `warm` of warm-up"""
    s.profile(True)
    for _ in range(warm):
        s.map_summary()
    k, w = [], []
    for _ in range(calls):
        a = s.kernel_time("map_summary")[0] + s.kernel_time("map_finish")[0]
        s.timer_start()
        ms = s.map_summary()
        w.append(s.timer_stop())
        k.append(s.kernel_time("map_summary")[0] + s.kernel_time("map_finish")[0] - a)
    s.profile(False)
    return k, w, ms


def describe(name, n, ms, k, w):
    slots = len(ms["share"])
    held = int((ms["holders"] > 0).sum())
    b = bytes_of(n, slots)
    km, wm = statistics.median(k), statistics.median(w)
    return ["%s" % name,
            "  slots %d (%d held by somebody, %d by every particle, %d with share >= 0.5)" % (slots, held, int((ms["holders"] == n).sum()), int((ms["share"] >= 0.5).sum())),
            "  kernels (map_summary + map_finish, all chunks)  %.4f ms  (calls %s)" % (km, " ".join("%.4f" % x for x in k)),
            "  whole call (launches, copies of the result, sync) %.4f ms  (calls %s)" % (wm, " ".join("%.4f" % x for x in w)),
            "  per (particle, slot): %.2f ps;  algorithmic bytes %.3f GB -> %.2f TB/s = %.0f %% of 8 TB/s (copy rate of this part: %.1f-%.1f TB/s)" %
            (1e9 * km / (n * slots), b / 1e9, b / (km * 1e-3) / 1e12, 100.0 * b / (km * 1e-3) / PEAK, COPY[0] / 1e12, COPY[1] / 1e12), ""]


def timed_pairs(s, pairs, calls=7, warm=2):
    """(kernel ms, whole-call ms, answer) of `calls` slamgpu_map_pairs over `pairs` after `warm` of warm-up"""
    s.profile(True)
    for _ in range(warm):
        s.map_pairs(pairs)
    k, w = [], []
    for _ in range(calls):
        a = s.kernel_time("map_pairs")[0] + s.kernel_time("map_finish")[0]
        s.timer_start()
        mp = s.map_pairs(pairs)
        w.append(s.timer_stop())
        k.append(s.kernel_time("map_pairs")[0] + s.kernel_time("map_finish")[0] - a)
    s.profile(False)
    return k, w, mp


def describe_pairs(name, n, s, pairs, how):
    from slam_amd import host
    ks, ws, ms = timed_summaries(s)
    slots = len(ms["share"])
    lines = [name]
    if len(pairs) == 0:
        return lines + ["  %s: none" % how, ""]
    k, w, mp = timed_pairs(s, pairs)
    km, wm, ksm = statistics.median(k), statistics.median(w), statistics.median(ks)
    b = 2.0 * (4.0 + 20.0) * n * len(pairs)
    mg = host.map_merge(ms, pairs, mp, 1.0, 0.1)
    sizes = np.bincount(mg["cluster"][mg["cluster"] >= 0], minlength=len(mg["merged"]))
    lines += ["  %d slots, %d pairs (%s); joint share: %d pairs 0, %d in (0, 0.1 min(s_a, s_b)], %d above; largest %.6f" %
              (slots, len(pairs), how, int((mp["share"] == 0).sum()),
               int(((mp["share"] > 0) & (mp["share"] <= 0.1 * np.minimum(ms["share"][pairs[:, 0]], ms["share"][pairs[:, 1]]))).sum()),
               int((mp["share"] > 0.1 * np.minimum(ms["share"][pairs[:, 0]], ms["share"][pairs[:, 1]])).sum()), float(np.nanmax(mp["share"]))),
              "  kernels (map_pairs + map_finish, all chunks)     %.4f ms  (calls %s)" % (km, " ".join("%.4f" % x for x in k)),
              "  whole call (copy of the list, launches, copies of the result, sync) %.4f ms  (calls %s)" % (wm, " ".join("%.4f" % x for x in w)),
              "  per (particle, record) read: %.2f ps;  slamgpu_map_summary of the %d slots on the same state, same process: kernels %.4f ms = %.2f ps per "
              "(particle, record) read" % (1e9 * km / (2.0 * n * len(pairs)), slots, ksm, 1e9 * ksm / (n * slots)),
              "  algorithmic bytes %.3f GB -> %.2f TB/s (copy rate of this part: %.1f-%.1f TB/s)" % (b / 1e9, b / (km * 1e-3) / 1e12, COPY[0] / 1e12, COPY[1] / 1e12),
              "  slamhost_map_merge (radius 1 m, cohold 0.1): %d slots with share > 0 -> %d landmarks, %d clusters of more than one slot (largest %d slots); "
              "share >= 0.5: %d slots -> %d landmarks" % (int((ms["share"] > 0).sum()), len(mg["merged"]), int((sizes > 1).sum()), int(sizes.max()) if len(sizes) else 0,
                                                          int((ms["share"] >= 0.5).sum()), int((mg["share"] >= 0.5).sum())), ""]
    return lines


def pairs_probe(out):
    from slam_amd import host
    lines = ["map_summary_probe --pairs: slamgpu_map_pairs, 10^5 particles, fast build; 2 calls of warm-up, median of 7", ""]
    web = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100)
    s = slam_amd.SlamGpu(N, web["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         math_mode=slam_amd.MATH_FAST)
    s.set_map(web["lm"])
    s.run_observe(web["ctl"], web["Q"], web["dt"], web["xt"], web["max_range"], web["R"], noise=2)
    s.history_fetch()
    nf = s.nf()
    pairs = np.array([(a, b) for a in range(nf) for b in range(a + 1, nf)], np.int32).reshape(-1, 2)
    lines += describe_pairs("(a) example_webmap, known association, compact genealogy, after 100 observation steps", N, s, pairs, "all a < b of the slots in use")
    s.close()
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 200)
    s = context(c5, N, 10000)
    device_steps(s, c5, 0, 200, dict(OPT, mode=slam_amd.capi.ASSOC_LISTS, excl=EXCL_OFF), 50)
    s.history_fetch()
    s.particle_report_fetch()
    pairs = host.map_candidates(s.map_summary(), 1.0)
    lines += describe_pairs("(b) config 5: synthetic 10^4-landmark map, per-particle association through the lists (run_particle), plain rows, log-weights, "
                            "after 200 steps", N, s, pairs, "all a < b with the posterior means within 1 m")
    s.close()
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


def trace(path):
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 220)
    s = context(c5, N, 10000)
    opt = dict(OPT, mode=slam_amd.capi.ASSOC_GRID, excl=EXCL_OFF)
    host_steps(s, c5, 0, 100, opt, 1)
    s.history_fetch()
    visited, launches, slots_seen = 0, 0, 0
    for k in range(100, 220):
        h = s.map_summary()["holders"]
        partial = int(((h > 0) & (h < N)).sum())
        slots_seen = len(h)
        visited += partial
        launches += partial > 0
        host_steps(s, c5, k, k + 1, opt, 1)
    s.history_fetch()
    s.close()
    out = dict(particles=N, steps=120, summaries=120, slots=slots_seen, census_launches_expected=int(launches), census_slots_visited=int(visited))
    with open(path, "w") as f:
        json.dump(out, f)
    print("trace run:", out)


def near_counts(xy, lm):
    """(true landmarks within 1 m of one of the points xy[k, 2], points within 1 m of no true landmark)"""
    hit = np.zeros(lm.shape[1], bool)
    stray = 0
    for x, y in xy:
        d = (lm[0] - x) ** 2 + (lm[1] - y) ** 2 < 1.0
        hit |= d
        stray += not d.any()
    return int(hit.sum()), stray


def tape():
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 100000)
    steps = len(c5["ctl"])
    s = context(c5, N, 15000)
    s.set_particle_excl_spacing(0.5)
    device_steps(s, c5, 0, steps, dict(OPT, mode=slam_amd.capi.ASSOC_LISTS, excl=EXCL_ON), 64)
    s.history_fetch()
    s.particle_report_fetch()
    lm = np.asarray(c5["lm"], np.float64).reshape(2, -1)
    w = s.peek(landmarks=False)["w"]
    ms = s.map_summary()
    best = int(np.argmax(w))
    xf = s.peek(first=best, count=1)["xf"][0].astype(np.float64)
    s.close()
    held = ~np.isnan(xf[:, 0])
    conf = ms["share"] >= 0.5
    cb, sb = near_counts(xf[held], lm)
    cp, sp = near_counts(ms["mean"][conf], lm)
    spread = np.sqrt(ms["scatter"][conf][:, 0] + ms["scatter"][conf][:, 2] + ms["pf"][conf][:, 0] + ms["pf"][conf][:, 2])
    return ["config 5, the whole tape: %d steps, 10^5 particles, run_particle(LISTS) K = 64, exclusion rule with the spacing cap f = 0.5, slot capacity 15 000, "
            "log-weights, fast build; %d slots in use" % (steps, len(ms["share"])),
            "  best particle (number %d)   landmarks %5d  true landmarks within 1 m of one of them %5d of %d  stray %4d" % (best, int(held.sum()), cb, lm.shape[1], sb),
            "  posterior (share >= 0.5)     slots     %5d  true landmarks within 1 m of a mean        %5d of %d  stray %4d   slots with share in (0, 0.5): %d, "
            "share 0: %d" % (int(conf.sum()), cp, lm.shape[1], sp, int(((ms["share"] > 0) & ~conf).sum()), int((ms["share"] == 0).sum())),
            "  total spread sqrt(tr(scatter + mean Pf)) of the confident slots: median %.3f m, 90 %% %.3f m, max %.3f m" %
            (float(np.median(spread)), float(np.quantile(spread, 0.9)), float(spread.max())), ""]


def summarize(stats_csv, counts_json):
    c = json.load(open(counts_json))
    rows = {}
    for r in csv.DictReader(open(stats_csv)):
        for key in ("pp_holders_kernel", "map_summary_kernel", "map_finish_kernel"):
            if key in r["Name"]:
                rows[key] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    n = c["particles"]
    lines = ["holders census beside the summary, one rocprofv3 --kernel-trace --stats run: config 5 driven by the host (slamgpu_update_particle, grid, census every "
             "step), 100 steps of warm-up, then %d steps with a summary of all %d slots before each" % (c["steps"], c["slots"])]
    if "pp_holders_kernel" in rows:
        calls, ns = rows["pp_holders_kernel"]
        lines.append("  pp_holders_kernel   %5d launches (whole run), %.1f us each" % (calls, ns / calls / 1e3))
        if c["census_slots_visited"]:
            per = c["census_slots_visited"] / max(c["census_launches_expected"], 1)
            lines.append("    in the %d counted steps: %d launches due, %d partial slots visited (%.1f per launch) -> ~%.0f ps per (particle, slot) visited at the "
                         "run's mean launch time" % (c["steps"], c["census_launches_expected"], c["census_slots_visited"], per, ns / calls * 1e3 / (n * per)))
    else:
        lines.append("  pp_holders_kernel   no launch in this run (no partial slot was due: %d expected)" % c["census_launches_expected"])
    if "map_summary_kernel" in rows:
        calls, ns = rows["map_summary_kernel"]
        fcalls, fns = rows.get("map_finish_kernel", (0, 0.0))
        per_summary = (ns + fns) / c["summaries"]
        lines.append("  map_summary_kernel  %5d launches (%d summaries, chunks of the partials' table), map_finish_kernel %d: %.3f ms per summary of %d slots "
                     "-> %.2f ps per (particle, slot) visited" % (calls, c["summaries"], fcalls, per_summary / 1e6, c["slots"], per_summary * 1e3 / (n * c["slots"])))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--summarize", nargs=2, default=None)
    ap.add_argument("--tape", action="store_true")
    ap.add_argument("--pairs", action="store_true")
    a = ap.parse_args()
    if a.pairs:
        if slam_amd.device_count() < 1:
            raise RuntimeError("map_summary_probe needs a GPU")
        pairs_probe(a.out)
        return
    if a.trace:
        trace(a.trace)
        return
    if a.tape:
        text = "\n".join(tape())
        print(text)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text)
        return
    if a.summarize:
        text = summarize(*a.summarize)
        print(text)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text)
        return
    if slam_amd.device_count() < 1:
        raise RuntimeError("map_summary_probe needs a GPU")
    lines = ["map_summary_probe: slamgpu_map_summary over all slots, 10^5 particles, fast build; 2 calls of warm-up, median of 7", ""]
    web = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100)
    s = slam_amd.SlamGpu(N, web["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         math_mode=slam_amd.MATH_FAST)
    s.set_map(web["lm"])
    s.run_observe(web["ctl"], web["Q"], web["dt"], web["xt"], web["max_range"], web["R"], noise=2)
    s.history_fetch()
    k, w, ms = timed_summaries(s)
    s.close()
    lines += describe("(a) example_webmap, known association, compact genealogy, after 100 observation steps", N, ms, k, w)
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 200)
    s = context(c5, N, 10000)
    device_steps(s, c5, 0, 200, dict(OPT, mode=slam_amd.capi.ASSOC_LISTS, excl=EXCL_OFF), 50)
    s.history_fetch()
    s.particle_report_fetch()
    k, w, ms = timed_summaries(s)
    s.close()
    lines += describe("(b) config 5: synthetic 10^4-landmark map, per-particle association through the lists (run_particle), plain rows, log-weights, "
                      "after 200 steps", N, ms, k, w)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
