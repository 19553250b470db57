"""Raw clouds through the three pieces (pipeline.detect_points: quantise call, torch gathers with the GIL held,
detect_scene_c) against the ONE C call (pipeline.detect_points_c), with one scene in flight and with seven scene threads.

    python profiles/points_call.py [--out profiles/quantize/points_call.txt] [--samples 300000] [--threads 1 7]

Raw fp32 clouds of synth.make_raw_scene (four seeds, cycled), 3 cm voxels, teacher predictions, MinkUNet34C(3, 64).  Per
thread count: every thread has its own stream and runs --scenes scenes per repeat; the two paths alternate, --repeats
repeats each, in this one process, after a warm-up of both.  Seven threads run under pipeline.policy_for_scenes_in_flight(7),
one thread under the library defaults - the same policy for both paths.  Reported per path: scenes/s of every repeat in run
order (wall clock from the common start to the last thread's stream synchronise), their median and spread (max - min), and
what a scene costs its calling thread: wall milliseconds and CPU microseconds of the thread (time.thread_time) per scene.
No profiler."""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = 0.03


def run_config(n_threads, paths, clouds, scenes, repeats, dev):
    """-> {path name: [(scenes/s, wall ms per scene and thread, thread CPU us per scene)] per repeat}, detections per cloud"""
    import torch

    from canonicalvoting_amd import pipeline
    policy = pipeline.policy_for_scenes_in_flight(n_threads)
    order = [name for _ in range(repeats) for name in paths]            # A B A B A B
    rounds = ["warm:" + name for name in paths] + order
    gate = threading.Barrier(n_threads + 1)
    stats = [[None] * len(rounds) for _ in range(n_threads)]
    errors, n_dets = [], {}

    def worker(i):
        try:
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                for k, what in enumerate(rounds):
                    fn = paths[what.split(":")[-1]]
                    count = 3 if what.startswith("warm:") else scenes
                    gate.wait()
                    w0, c0 = time.perf_counter(), time.thread_time()
                    for s in range(count):
                        j = (i + s) % len(clouds)
                        out = fn(clouds[j], policy)
                        n_dets.setdefault((what.split(":")[-1], j), len(out[0]))
                    c1 = time.thread_time()
                    stream.synchronize()
                    stats[i][k] = ((time.perf_counter() - w0) / count, (c1 - c0) / count)
                    gate.wait()
        except BaseException as e:      # noqa: BLE001
            errors.append(repr(e))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(n_threads)]
    for t in threads:
        t.start()
    result = {name: [] for name in paths}
    try:
        for k, what in enumerate(rounds):
            gate.wait()
            t0 = time.perf_counter()
            gate.wait()
            wall = time.perf_counter() - t0
            if not what.startswith("warm:"):
                per = [stats[i][k] for i in range(n_threads)]
                result[what].append((n_threads * scenes / wall, 1e3 * statistics.mean(p[0] for p in per),
                                     1e6 * statistics.mean(p[1] for p in per)))
    except threading.BrokenBarrierError:
        pass
    for t in threads:
        t.join()
    if errors:
        sys.exit("points_call: a scene thread failed, nothing more is started: %s" % errors[0])
    return result, n_dets, order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize", "points_call.txt"))
    ap.add_argument("--samples", type=int, default=300000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 7])
    ap.add_argument("--scenes", type=int, default=10, help="scenes per thread and repeat")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--append", nargs="*", default=[], help="text files appended to the report (the bench.py lines of the same job)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from canonicalvoting_amd import pipeline
    from canonicalvoting_amd.hough import HoughVoting
    from canonicalvoting_amd.minkunet import MinkUNet34C
    from canonicalvoting_amd.synth import make_raw_scene, synth_predictions
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    sys.setswitchinterval(0.0005)            # (bench.py's setting for its scene threads)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(dev).eval()
    hv = HoughVoting(RES, 120)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    clouds = []
    for seed in range(4):
        raw = make_raw_scene(seed, a.samples)
        clouds.append((t(raw.points.astype(np.float32)), t((raw.feats * 2 - 1).astype(np.float32)),
                       tuple(t(x) for x in synth_predictions(raw))))
    torch.cuda.synchronize()
    paths = {
        "detect_points": lambda c, pol: pipeline.detect_points(model, hv, c[0], c[1], RES, predictions=c[2], policy=pol, thresh_high=60),
        "detect_points_c": lambda c, pol: pipeline.detect_points_c(model, hv, c[0], c[1], RES, predictions=c[2], policy=pol,
                                                                   thresh_high=60),
    }
    voxels = [int(pipeline.detect_points_c(model, hv, c[0], c[1], RES, predictions=c[2], thresh_high=60)[3].shape[0]) for c in clouds]
    lines = ["raw clouds, three pieces (detect_points) against one C call (detect_points_c): fp32 clouds of synth.make_raw_scene(seed, %d),"
             % a.samples, "seeds 0-3 cycled (%s voxels at %.2f m), teacher predictions, MinkUNet34C(3, 64); %d repeats of %d scenes per thread,"
             % (" / ".join(str(v) for v in voxels), RES, a.repeats, a.scenes), "the two paths alternated in one process after a warm-up of both", ""]
    med = statistics.median
    for n_threads in a.threads:
        result, n_dets, order = run_config(n_threads, paths, clouds, a.scenes, a.repeats, dev)
        same = all(n_dets.get(("detect_points", j)) == n_dets.get(("detect_points_c", j)) for j in range(len(clouds)))
        lines.append("%d scene thread%s (%s), run order %s; detections per cloud equal: %s" %
                     (n_threads, "" if n_threads == 1 else "s", "library launch sizing" if n_threads < 4 else "in-flight launch sizing",
                      " ".join("P" if o == "detect_points" else "C" for o in order), "yes" if same else "NO"))
        for name in paths:
            rate = [r[0] for r in result[name]]
            lines.append("  %-16s scenes/s %s   median %.2f   spread (max - min) %.2f" %
                         (name, " ".join("%.2f" % r for r in rate), med(rate), max(rate) - min(rate)))
            lines.append("  %-16s per scene and calling thread: wall %.3f ms, thread CPU %.0f us (medians of the repeats)" %
                         ("", med(r[1] for r in result[name]), med(r[2] for r in result[name])))
        p, c = [r[0] for r in result["detect_points"]], [r[0] for r in result["detect_points_c"]]
        spread = max(max(p) - min(p), max(c) - min(c))
        diff = med(c) - med(p)
        lines.append("  one call - three pieces: %+.2f scenes/s (%+.1f %%); the larger spread between repeats is %.2f: %s" %
                     (diff, 100 * diff / med(p), spread, "inside it" if abs(diff) <= spread else ("faster" if diff > 0 else "SLOWER")))
        lines.append("")
    for path in a.append:
        with open(path) as f:
            lines += [f.read().rstrip(), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
