"""Record tests/golden/f64_digests.json: the SHA-256 of what a build's float64 tile kernels return for the cases of
tests/test_gpu_f64_digests.py, through the public Python API.

    BBBP_LIB=/path/to/reference/libbbbp_hip.so python tools/record_f64_digests.py [--check]

The reference is a build of the commit a refactor of csrc/f64_tile.h, pca.hip or knn.hip starts from, not the working tree.  --check compares
instead of writing (exit status 1 on a difference).  Needs the GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    if not os.environ.get("BBBP_LIB"):
        raise SystemExit("set BBBP_LIB to the reference build's libbbbp_hip.so")
    import test_gpu_f64_digests as T
    rows = {g: T.compute_digests(g) for g in T.GROUPS}
    text = json.dumps(rows, indent=1) + "\n"
    count = sum(len(v) for v in rows.values())
    if "--check" in sys.argv:
        with open(T.DIGESTS) as f:
            same = f.read() == text
        print("f64 digests:", "identical" if same else "DIFFERENT", f"({count} outputs)")
        raise SystemExit(0 if same else 1)
    with open(T.DIGESTS, "w") as f:
        f.write(text)
    print(f"wrote {T.DIGESTS}: {count} outputs")


if __name__ == "__main__":
    main()
