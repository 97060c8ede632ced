"""slam-backend's command-line contract, as recorded from the driver of the commit before its sources were split
(tests/golden/backend_cli_parent.json): for every command line of CASES the exit status, stdout and stderr of the built binary equal the
recorded ones.  The cases are -h, every refusal that ends the program before a device call (each message at least once), command lines
that break two rules at once (which message wins), runs that pass every check and then fail for want of a device (flagged "no_device";
skipped where there is one) and two complete host-EKF runs, whose -log is compared on its first seven columns (the eighth is a time).
One normalisation: the number in `mean loop time <number> us`.

The fixture is a recording, not a second build: a checkout need not carry the history to build the parent's driver from.  It was taken
on a machine without a GPU by this module itself from the parent's binary (commit 7ace5e4):
python tests/test_backend_cli_cpu.py slam_amd/bin/slam-backend > tests/golden/backend_cli_parent.json
The data directory, the executable and the temporary directory are written as {DATA}, {EXE} and {TMP}."""
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
PARENT = os.path.join(ROOT, "tests", "golden", "backend_cli_parent.json")
LOOP_TIME = re.compile(r"mean loop time [0-9.eE+-]+ us")

BASE = ["-m", "{DATA}/example_webmap.mat", "-NPARTICLES", "512", "-SWITCH_SEED_RANDOM", "7", "-maxsteps", "300"]
FS2 = BASE + ["-method", "FASTSLAM2"]
EKF = BASE + ["-method", "EKF1"]
DEV = EKF + ["-ekf", "device"]
ENS = DEV + ["-runs", "8"]


def _c(name, args, **kw):
    return dict(name=name, args=args, **kw)


CASES = [
    _c("help", ["-h"]),
    # Simulator::init
    _c("init_no_map_file", ["-m", "{TMP}/absent.mat", "-method", "EKF1"]),
    # refusals from the arguments alone, in the order the driver makes them
    _c("map_word", FS2 + ["-map", "all"]),
    _c("joint_out_without_joint", FS2 + ["-map", "posterior", "-JOINT_OUT", "{TMP}/j.txt"]),
    _c("joint_out_without_map", FS2 + ["-JOINT_OUT", "{TMP}/j.txt"]),
    _c("map_joint_ekf", EKF + ["-map", "joint"]),
    _c("ekf_word", EKF + ["-ekf", "gpu"]),
    _c("ekf_device_fastslam", FS2 + ["-ekf", "device"]),
    _c("runs_fastslam", FS2 + ["-runs", "8"]),
    _c("runs_host_ekf", EKF + ["-runs", "8"]),
    _c("runs_plot", ENS + ["-plot", "file:{TMP}/f.bin"]),
    _c("runs_zero", DEV + ["-runs", "0"]),
    _c("runs_too_many", DEV + ["-runs", "65536"]),
    _c("runs_seed_alone", EKF + ["-RUNS_SEED", "3"]),
    _c("local_host_ekf", EKF + ["-EKF_LOCAL", "20"]),
    _c("local_fastslam", FS2 + ["-EKF_LOCAL", "20"]),
    _c("local_runs", ENS + ["-EKF_LOCAL", "20"]),
    _c("local_margin", DEV + ["-EKF_LOCAL", "0"]),
    _c("local_new_alone", DEV + ["-EKF_LOCAL_NEW", "8"]),
    _c("local_new_zero", DEV + ["-EKF_LOCAL", "20", "-EKF_LOCAL_NEW", "0"]),
    _c("runs_batch_alone", DEV + ["-RUNS_BATCH", "4"]),
    _c("runs_batch_zero", ENS + ["-RUNS_BATCH", "0"]),
    _c("runs_batch_large", ENS + ["-RUNS_BATCH", "4097"]),
    _c("runs_trace_alone", DEV + ["-RUNS_TRACE", "{TMP}/t.txt"]),
    _c("runs_moments_alone", DEV + ["-RUNS_MOMENTS", "1"]),
    _c("runs_moments_zero_alone", EKF + ["-RUNS_MOMENTS", "0"]),
    _c("runs_moments_out_alone", ENS + ["-RUNS_MOMENTS_OUT", "{TMP}/m.txt"]),
    _c("runs_moments_out_off", ENS + ["-RUNS_MOMENTS", "0", "-RUNS_MOMENTS_OUT", "{TMP}/m.txt"]),
    _c("merge_radius_without_merged", FS2 + ["-map", "posterior", "-MAP_MERGE_RADIUS", "2"]),
    _c("merge_cohold_without_map", FS2 + ["-MAP_MERGE_COHOLD", "0.2"]),
    _c("merge_radius_zero", FS2 + ["-map", "merged", "-MAP_MERGE_RADIUS", "0"]),
    _c("merge_cohold_large", FS2 + ["-map", "merged", "-MAP_MERGE_COHOLD", "1.5"]),
    _c("path_word", FS2 + ["-path", "all"]),
    _c("path_records_zero", FS2 + ["-path", "smoothed", "-PATH_RECORDS", "0"]),
    _c("path_ekf", EKF + ["-path", "smoothed"]),
    _c("path_gpus", FS2 + ["-path", "smoothed", "-gpus", "2"]),
    _c("path_particle_device", FS2 + ["-path", "smoothed", "-assoc", "particle", "-observe", "device"]),
    _c("pose_word", FS2 + ["-pose", "all"]),
    _c("pose_records_zero", FS2 + ["-pose", "posterior", "-POSE_RECORDS", "0"]),
    _c("pose_ekf", EKF + ["-pose", "posterior"]),
    _c("pose_gpus", FS2 + ["-pose", "posterior", "-gpus", "2"]),
    _c("pose_records_alone", FS2 + ["-POSE_RECORDS", "16"]),
    _c("pose_records_with_none", FS2 + ["-pose", "none", "-POSE_RECORDS", "16"]),
    _c("innovation_word", FS2 + ["-innovation", "all"]),
    _c("innovation_records_zero", FS2 + ["-innovation", "posterior", "-INNOVATION_RECORDS", "0"]),
    _c("innovation_ekf", EKF + ["-innovation", "posterior"]),
    _c("innovation_gpus", FS2 + ["-innovation", "posterior", "-gpus", "2"]),
    _c("innovation_observe_device", FS2 + ["-innovation", "posterior", "-observe", "device"]),
    _c("innovation_particle", FS2 + ["-innovation", "posterior", "-assoc", "particle"]),
    _c("innovation_records_alone", FS2 + ["-INNOVATION_RECORDS", "16"]),
    # ... after the settings are printed
    _c("plot_sink", FS2 + ["-plot", "screen"]),
    _c("plot_tcp_without_port", EKF + ["-plot", "tcp://127.0.0.1"]),
    _c("plot_file_in_no_directory", EKF + ["-plot", "file:{TMP}/absent/f.bin"]),
    _c("gpus_map_posterior", FS2 + ["-gpus", "2", "-map", "posterior"]),
    _c("gpus_map_merged", FS2 + ["-gpus", "2", "-map", "merged"]),
    _c("gpus_map_joint", FS2 + ["-gpus", "2", "-map", "joint"]),
    _c("gpus_log_weights", FS2 + ["-gpus", "2", "-LOG_WEIGHTS", "1"]),
    _c("gpus_parity", FS2 + ["-gpus", "2", "-rng", "parity"]),
    _c("gpus_gated", FS2 + ["-gpus", "2", "-assoc", "gated"]),
    _c("gpus_particle", FS2 + ["-gpus", "2", "-assoc", "particle"]),
    _c("gpus_zero", FS2 + ["-gpus", "0"]),
    _c("gpus_multiple", FS2 + ["-gpus", "3"]),
    _c("gpus_refusal_ends_the_plot", FS2 + ["-gpus", "3", "-plot", "file:{TMP}/f.bin"]),
    _c("observe_device_ekf", EKF + ["-observe", "device"]),
    _c("observe_device_parity", FS2 + ["-observe", "device", "-rng", "parity"]),
    _c("observe_device_gated", FS2 + ["-observe", "device", "-assoc", "gated"]),
    _c("observe_device_plot", FS2 + ["-observe", "device", "-plot", "file:{TMP}/f.bin"]),
    _c("observe_device_loop_step", FS2 + ["-observe", "device", "-loop", "step"]),
    _c("miss_alone", FS2 + ["-assoc", "particle", "-PARTICLE_MISS", "0.5"]),
    _c("miss_margin_alone", FS2 + ["-assoc", "particle", "-PARTICLE_MISS_MARGIN", "2"]),
    _c("miss_without_particle", FS2 + ["-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "2"]),
    _c("miss_ekf", EKF + ["-assoc", "particle", "-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "2"]),
    _c("miss_p_zero", FS2 + ["-assoc", "particle", "-PARTICLE_MISS", "0", "-PARTICLE_MISS_MARGIN", "2"]),
    _c("miss_margin_beyond_range", FS2 + ["-assoc", "particle", "-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "60"]),
    _c("log_weights_ekf", EKF + ["-LOG_WEIGHTS", "1"]),
    _c("log_weights_word", FS2 + ["-LOG_WEIGHTS", "2"]),
    _c("particle_assoc_word", FS2 + ["-assoc", "particle", "-PARTICLE_ASSOC", "table"]),
    # two rules broken at once: which message wins
    _c("two_pose_gpus_before_gpus_map_joint", FS2 + ["-pose", "posterior", "-gpus", "2", "-map", "joint", "-JOINT_OUT", "{TMP}/j.txt"]),
    _c("two_map_word_before_ekf_word", FS2 + ["-ekf", "gpu", "-map", "all"]),
    _c("two_joint_out_before_ekf_word", FS2 + ["-ekf", "gpu", "-map", "posterior", "-JOINT_OUT", "{TMP}/j.txt"]),
    _c("two_map_joint_ekf_before_plot_sink", EKF + ["-plot", "screen", "-map", "joint"]),
    _c("two_ekf_device_fastslam_before_runs", FS2 + ["-runs", "8", "-ekf", "device"]),
    _c("two_runs_before_local", EKF + ["-EKF_LOCAL", "20", "-runs", "8", "-RUNS_SEED", "3"]),
    _c("two_runs_plot_before_count", DEV + ["-runs", "0", "-plot", "file:{TMP}/f.bin"]),
    _c("two_local_runs_before_margin", ENS + ["-EKF_LOCAL", "0"]),
    _c("two_local_new_alone_before_zero", DEV + ["-EKF_LOCAL_NEW", "0"]),
    _c("two_runs_batch_alone_before_zero", DEV + ["-RUNS_BATCH", "0", "-RUNS_TRACE", "{TMP}/t.txt"]),
    _c("two_merge_before_path", FS2 + ["-path", "all", "-MAP_MERGE_RADIUS", "2"]),
    _c("two_path_records_before_ekf", EKF + ["-path", "smoothed", "-PATH_RECORDS", "0"]),
    _c("two_path_before_pose", EKF + ["-pose", "all", "-path", "smoothed"]),
    _c("two_pose_before_innovation", FS2 + ["-innovation", "all", "-POSE_RECORDS", "16"]),
    _c("two_innovation_observe_device_before_particle", FS2 + ["-innovation", "posterior", "-assoc", "particle", "-observe", "device"]),
    _c("two_plot_sink_before_gpus_map", FS2 + ["-gpus", "2", "-map", "joint", "-plot", "screen"]),
    _c("two_gpus_map_before_log_weights", FS2 + ["-gpus", "2", "-LOG_WEIGHTS", "1", "-map", "merged"]),
    _c("two_gpus_log_weights_before_parity", FS2 + ["-gpus", "2", "-rng", "parity", "-LOG_WEIGHTS", "1"]),
    _c("two_gpus_parity_before_zero", FS2 + ["-gpus", "0", "-rng", "parity"]),
    _c("two_gpus_zero_before_multiple", BASE[:2] + ["-NPARTICLES", "100", "-method", "FASTSLAM2", "-gpus", "0"]),
    _c("two_observe_device_before_miss", FS2 + ["-PARTICLE_MISS", "0.5", "-observe", "device", "-rng", "parity"]),
    _c("two_miss_before_log_weights", FS2 + ["-LOG_WEIGHTS", "2", "-PARTICLE_MISS", "0.5"]),
    _c("two_log_weights_before_particle_assoc", FS2 + ["-PARTICLE_ASSOC", "table", "-LOG_WEIGHTS", "2"]),
    # every check passed, then no device (skipped where there is one)
    _c("no_device_fastslam", FS2, no_device=True),
    _c("no_device_particle_mutex_without_particle", FS2 + ["-PARTICLE_MUTEX", "1"], no_device=True),
    _c("no_device_path_records_without_path", FS2 + ["-PATH_RECORDS", "16"], no_device=True),
    _c("no_device_ekf", DEV, no_device=True),
    _c("no_device_ekf_local", DEV + ["-EKF_LOCAL", "20", "-EKF_LOCAL_NEW", "8"], no_device=True),
    _c("no_device_runs", ENS, no_device=True),
    _c("no_device_runs_options", ENS + ["-RUNS_SEED", "3", "-RUNS_BATCH", "4", "-RUNS_TRACE", "{TMP}/t.txt", "-RUNS_MOMENTS", "1", "-RUNS_MOMENTS_OUT",
                                        "{TMP}/m.txt"], no_device=True),
    _c("no_device_gpus", FS2 + ["-gpus", "2"], no_device=True),
    # complete runs of the host EKF
    _c("host_ekf_known", EKF + ["-log", "{TMP}/log.csv"], log=True),
    _c("host_ekf_gated", EKF + ["-SWITCH_ASSOCIATION_KNOWN", "0", "-log", "{TMP}/log.csv"], log=True),
    _c("host_ekf_keys_that_only_fastslam_reads", EKF + ["-PATH_RECORDS", "16", "-maxsteps", "40", "-log", "{TMP}/log.csv"], log=True),
]


def run_case(case, exe):
    """status, stdout, stderr (and the log's first seven columns) of one case, the machine's paths written as placeholders"""
    with tempfile.TemporaryDirectory() as tmp:
        places = (("{TMP}", tmp), ("{DATA}", DATA), ("{EXE}", exe))

        def real(s):
            for k, v in places:
                s = s.replace(k, v)
            return s

        def placeholder(s):
            for k, v in places:
                s = s.replace(v, k)
            return LOOP_TIME.sub("mean loop time # us", s)

        p = subprocess.run([exe] + [real(a) for a in case["args"]], capture_output=True, text=True, timeout=60)
        got = {"status": p.returncode, "stdout": placeholder(p.stdout), "stderr": placeholder(p.stderr)}
        if case.get("log"):
            got["log"] = [",".join(ln.rstrip("\n").split(",")[:7]) for ln in open(os.path.join(tmp, "log.csv"))]
        return got


def _recorded():
    return json.load(open(PARENT))


def test_the_fixture_holds_exactly_these_cases():
    rec = _recorded()
    assert [c["name"] for c in rec] == [c["name"] for c in CASES]
    assert len({c["name"] for c in CASES}) == len(CASES)
    for r, c in zip(rec, CASES):
        assert r["args"] == c["args"] and bool(r.get("no_device")) == bool(c.get("no_device")), c["name"]
    # a refusal is one line on stderr and a failure status; only the help and the complete runs end well
    assert [r["name"] for r in rec if r["status"] == 0] == ["help"] + [c["name"] for c in CASES if c.get("log")]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_backend_answers_as_the_parent_did(case):
    if case.get("no_device"):
        import slam_amd
        if slam_amd.device_count() > 0:
            pytest.skip("recorded without a device: with one this command line runs")
    want = next(r for r in _recorded() if r["name"] == case["name"])
    got = run_case(case, EXE)
    print(got["stderr"], got["stdout"][-400:])
    assert got["status"] == want["status"]
    assert got["stderr"] == want["stderr"]
    assert got["stdout"] == want["stdout"]
    if case.get("log"):
        assert got["log"] == want["log"]


if __name__ == "__main__":  # the fixture: see the module's docstring
    print(json.dumps([dict(c, **run_case(c, os.path.abspath(sys.argv[1]))) for c in CASES], indent=0))
