"""Bitwise parity of two builds of libmss_hip.so on every case of tests/test_gpu_fwd_route.py (needs the GPU).

    python tools/fwd_route_parity.py outputs OTHER_LIB        # SHA-256 of every case's output, this tree's build against OTHER_LIB

Each build is loaded in a fresh child process (MSS_LIB chooses the library before the first import). Exits non-zero when a digest or a
route code differs. profiles/fwd_route/README.md holds the recorded result; tools/fwd_route_query_bench.cpp times the route query."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

def child_outputs():
    import test_gpu_fwd_route as t
    out = {}
    for name in t.CASES:
        code, y, _, _ = t.launch(name)
        out[name] = [code, hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()]
    print(json.dumps(out))


def run_child(mode, lib):
    env = dict(os.environ)
    env.pop("MSS_LIB", None)
    if lib:
        env["MSS_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child_" + mode], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"child ({lib or 'this tree'}) failed with {p.returncode}:\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().split("\n")[-1])


def main():
    mode = sys.argv[1]
    if mode == "child_outputs":
        return child_outputs()
    other = sys.argv[2]
    assert mode == "outputs"
    theirs, ours = run_child("outputs", other), run_child("outputs", None)
    bad = [n for n in ours if ours[n] != theirs.get(n)]
    for n in ours:
        print(f"{n:36s} code {ours[n][0]}  {ours[n][1][:16]}  {'equal' if n not in bad else 'DIFFERENT: other ' + str(theirs.get(n))}")
    print(f"{len(ours) - len(bad)} of {len(ours)} cases bitwise equal")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
