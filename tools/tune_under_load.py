"""Plan search under load: the autotuner times every alternative alone on the GPU, but the pipeline runs three forwards side by
side, where LDS footprint and occupancy of one kernel change what its neighbours get.  Greedy coordinate descent over the lines
of a plan file (profiles/plan_lite0.b64.f0), scored by end-to-end frames/s of the depth-3 pipeline:
    python tools/tune_under_load.py <plan_in> <plan_out>
Candidate edits are (line number, replacement text) pairs - same alternative with another variant, or another alternative
with the same number of steps.  A plan the library rejects (load_plan fails -> it would autotune) is detected by the
library re-writing the file and is skipped."""
import os, sys, time, shutil
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")
import numpy as np, torch
import bench
from vbt_amd.track import Pipeline
from vbt_amd.container import Container

plan_in, plan_out = sys.argv[1], sys.argv[2]
n = int(os.environ.get("TUL_BATCH", "64"))      # clips per step; the trial plan is written for this batch
KSTEPS = int(os.environ.get("TUL_STEPS", str(max(300, 19200 // n))))
SUF = f".b{n}.f0"
size = int(Container(bench.MODEL).header["image_size"])
U = 16
frames = torch.from_numpy(bench.make_frames(list(range(n)), 0, U, size)).cuda()
fbytes = frames[0].numel()
stream = torch.cuda.current_stream().cuda_stream
TRIAL = "/tmp/plan_trial"


def score(lines, reps=2, K=KSTEPS):
    with open(TRIAL + SUF, "w") as f:
        f.write("\n".join(lines) + "\n")
    before = open(TRIAL + SUF).read()
    os.environ["VBT_PLAN_FILE"] = TRIAL
    try:
        pipe = Pipeline(bench.MODEL, n, max_frames=K + 40, fps=60.0, detection_treshold=0.5, device=0, rows_per_frame=8)
    except Exception as e:                              # the creation-time self-check rejects the plan
        print(f"    rejected: {str(e)[:90]}", flush=True)
        torch.cuda.synchronize()
        return None
    if open(TRIAL + SUF).read() != before:
        del pipe
        return None                                  # the library did not accept the plan and re-tuned
    best = 0.0
    try:
        for _ in range(reps):
            pipe.reset()
            for i in range(20):
                pipe.step(frames.data_ptr() + (i % U) * fbytes, stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(K):
                pipe.step(frames.data_ptr() + (i % U) * fbytes, stream)
            pipe._drain()
            torch.cuda.synchronize()
            best = max(best, n * K / (time.perf_counter() - t0))
    except Exception as e:                              # a variant the kernel family does not offer for this layer
        print(f"    rejected: {str(e)[:90]}", flush=True)
        torch.cuda.synchronize()
        best = None
    del pipe
    return best


lines = open(plan_in).read().split("\n")
while lines and not lines[-1]:
    lines.pop()
if lines and lines[0].startswith("VBTPLAN2"):      # format 2 names the kernel families: the search edits bare indices (format 1, still
    lines[0] = lines[0].split()[1]                 # loadable); re-create the library once with VBT_PLAN_CONVERT=1 to get the names back
    lines[1:] = [" ".join(tok.rsplit(":", 1)[-1] for tok in ln.split()) for ln in lines[1:]]
# candidates: (1-based line, [texts])
cands = []
for ln, text in enumerate(lines, 1):
    t = text.split()
    if ln == 1:
        continue
    alt, ns, var = int(t[0]), int(t[1]), [int(x) for x in t[2:]]
    opts = set()
    if ns == 1 and var[0] in (1, 9, 17, 25, 0, 3, 11):           # fused tile kernels: other variants of the same alternative
        for v in (1, 9, 17, 25):
            opts.add(f"{alt} 1 {v}")
        for a2 in (alt - 1, alt + 1):                            # neighbouring alternative with one step (tile <-> band)
            if a2 >= 0:
                opts.add(f"{a2} 1 -1"); opts.add(f"{a2} 1 1")
    elif ns == 1 and var[0] == -1 and alt >= 2:
        opts.add(f"{alt - 1} 1 1")
    elif ns == 2 and var[0] % 100 in (1, 2, 3, 4, 6, 9, 18):      # expand + depthwise: chunks per workgroup x kernel form
        for form in (0, 100, 200, 300):                          # first form / second form on 8 waves / on 16 waves / its small-map instantiation
            for c in (1, 2, 3, 4, 6) + ((9, 18) if form else ()):
                opts.add(f"{alt} 2 {form + c} {var[1]}")
        for v in (-1, 2, 3, 4):                                  # the projection behind it: K-streaming / split-K / weights through LDS (64 / 128 pixels)
            opts.add(f"{alt} 2 {var[0]} {v}")
    opts.discard(text)
    if opts:
        cands.append((ln, sorted(opts)))

base = score(lines)
print(f"baseline {base:.0f} frames/s", flush=True)
for ln, opts in cands:
    for o in opts:
        trial = list(lines)
        trial[ln - 1] = o
        s = score(trial)
        if s is None:
            continue
        tag = ""
        if s > base * 1.003:
            s2 = score(trial)                                     # confirm
            if s2 is not None and s2 > base * 1.003:
                lines, base, tag = trial, max(s, s2), "  <- accepted"
                with open(plan_out, "w") as f:                    # (kept current: a search cut short by a time limit still leaves its best plan)
                    f.write("\n".join(lines) + "\n")
        print(f"line {ln:2d}: '{o}' {s:.0f}{tag}", flush=True)
with open(plan_out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"final {base:.0f} frames/s -> {plan_out}", flush=True)
