"""Bitwise parity of two builds of libmss_hip.so on the grid-from-the-device-cache launches of tests/test_gpu_device_state.py (needs the GPU).

    python tools/device_state_parity.py outputs OTHER_LIB     # SHA-256 of every output, this tree's build against OTHER_LIB
    python tools/device_state_parity.py record OTHER_LIB      # write OTHER_LIB's digests to tests/golden/device_state_parent.json

Each build is loaded in a fresh child process (MSS_LIB chooses the library before the first import), as tools/fwd_route_parity.py does.
`outputs` exits non-zero when a digest differs. profiles/device_state/README.md holds the recorded result."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "device_state_parent.json")


def run_child(lib):
    env = dict(os.environ)
    env.pop("MSS_LIB", None)
    if lib:
        env["MSS_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"child ({lib or 'this tree'}) failed with {p.returncode}:\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().split("\n")[-1])


def main():
    mode = sys.argv[1]
    if mode == "child":
        import test_gpu_device_state as t
        print(json.dumps({name: t.digest(y) for name, y in t.same_grid_outputs().items()}))
        return
    theirs = run_child(sys.argv[2])
    if mode == "record":
        with open(GOLDEN, "w") as f:
            json.dump(theirs, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {GOLDEN}")
        return
    assert mode == "outputs"
    ours = run_child(None)
    bad = [n for n in ours if ours[n] != theirs.get(n)]
    for n in ours:
        print(f"{n:16s} {ours[n][:16]}  {'equal' if n not in bad else 'DIFFERENT: other ' + str(theirs.get(n))}")
    print(f"{len(ours) - len(bad)} of {len(ours)} outputs bitwise equal")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
