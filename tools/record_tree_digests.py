"""Record tests/golden/tree_digests.json: the SHA-256 of what a commit's tree learners (gradient_boosting, random_forest) fit and predict
for the cases of tests/test_gpu_tree_digests.py, through the public Python API.

    python tools/record_tree_digests.py --package-root /path/to/checkout/of/the/starting/commit [--check]

The package root is a checkout (a ``git worktree``) of the commit a refactor of the tree learners starts from, with its own build of
libbbbp_hip.so: its Python and its kernels produce the record, this tree supplies only the cases.  --check compares instead of writing
(exit status 1 on a difference); without --package-root it checks this tree, which is what the test does.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", help="the checkout whose bbbp_amd package and build are recorded")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if not a.package_root and not a.check:
        raise SystemExit("give --package-root: the record comes from the commit a refactor starts from, not from this tree")
    package_root = os.path.abspath(a.package_root or ROOT)
    sys.path[:0] = [package_root, os.path.join(ROOT, "tests")]
    import bbbp_amd
    import test_gpu_tree_digests as T
    if not os.path.abspath(bbbp_amd.__file__).startswith(package_root + os.sep):
        raise SystemExit(f"bbbp_amd was imported from {bbbp_amd.__file__}, not from {package_root}")
    rows = {g: T.compute_digests(g) for g in T.GROUPS}
    text = json.dumps(rows, indent=1) + "\n"
    count = sum(len(v) for v in rows.values())
    if a.check:
        with open(T.DIGESTS) as f:
            same = f.read() == text
        print("tree digests:", "identical" if same else "DIFFERENT", f"({count} results, package {package_root})")
        raise SystemExit(0 if same else 1)
    with open(T.DIGESTS, "w") as f:
        f.write(text)
    print(f"wrote {T.DIGESTS}: {count} results of {package_root}")


if __name__ == "__main__":
    main()
