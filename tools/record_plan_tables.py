"""Record tests/plan_tables.json: what the plan functions of a build answer for the cases tests/test_plan_tables.py lists.

    BBBP_LIB=/path/to/reference/libbbbp_hip.so python tools/record_plan_tables.py [--check]

The reference is a build of the commit a refactor of the plan code starts from, not the working tree.  --check compares instead of writing
(exit status 1 on a difference).  No GPU is needed: without a device the library plans for 256 CUs, as on an MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_plan_tables as T  # noqa: E402


def main():
    path = os.environ.get("BBBP_LIB")
    if not path:
        raise SystemExit("set BBBP_LIB to the reference build's libbbbp_hip.so")
    rows = T.compute_tables(T.load_library(path))
    text = "{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r) for r in rows[k]) + "\n ]" for k in ("gemm", "conv")) + "\n}\n"
    if "--check" in sys.argv:
        same = open(T.TABLE).read() == text
        print("plan tables:", "identical" if same else "DIFFERENT", f"({len(rows['gemm'])} GEMM rows, {len(rows['conv'])} conv rows)")
        raise SystemExit(0 if same else 1)
    with open(T.TABLE, "w") as f:
        f.write(text)
    print(f"wrote {T.TABLE}: {len(rows['gemm'])} GEMM rows, {len(rows['conv'])} conv rows")


if __name__ == "__main__":
    main()
