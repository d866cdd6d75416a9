"""Where does the first timed block of the plain bench go?  (tools/first_launch_probe.py plain | fitfirst)  bench.py's own population and stepper, blocks split into
run(20)+sync and fitness+sync.  argv[1]: plain | fitfirst (one env.fitness read after warm-up, before the timed blocks)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import bench  # noqa: E402
mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
prep = bench.build_population("lsystem", 65536, 0)
morphs, _ = bench.finish_population(prep)
import torch  # noqa: E402
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
env = bench.make_env(morphs, dev, False, True, False)
run = bench.stepper(env, 50)
run(60)
run(5)
torch.cuda.synchronize()
if mode == "fitfirst":
    _ = env.fitness
    torch.cuda.synchronize()
out = []
for i in range(6):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(20)
    tq = time.perf_counter()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _ = env.fitness
    tf = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out.append({"block": i, "enqueue_ms": round((tq - t0) * 1e3, 3), "run_sync_ms": round((t1 - t0) * 1e3, 3),
                "fitness_call_ms": round((tf - t1) * 1e3, 3), "fitness_sync_ms": round((t2 - t1) * 1e3, 3)})
print(json.dumps({"mode": mode, "blocks": out}))
