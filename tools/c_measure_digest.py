"""Reduce the `c-measure <op> <dtype> <value>` lines of a GPU test log (pytest -s) to the worst value per
output and input kind, as quoted in DESIGN.md section 2.3.

    python -m pytest tests/test_gpu_convbn.py -q -s > log.txt
    python tools/c_measure_digest.py log.txt > profiles/<tag>_convbn_c_measure.txt
"""
import collections
import re
import sys


def main(path):
    worst, n = collections.defaultdict(float), 0
    for line in open(path):
        if not line.startswith("c-measure"):
            continue
        n += 1
        parts = line.split()
        val, dt, name = float(parts[-1]), parts[-2], " ".join(parts[1:-2])
        m = re.match(r"bn\[(\w+) M\d+ C\d+ (\w+) .*\]\.(\w+)", name)
        key = (f"bn.{m.group(3)} [{m.group(2)}]" if m else name, dt)
        worst[key] = max(worst[key], val)
    print(f"# worst `c-measure` value per output and input kind over {n} measurements of {path.split('/')[-1]}")
    print("# (error of the float32 CPU restatement against float64, in units of 2^-23 * scale; the tests use 4x, floor 16)")
    for k in sorted(worst):
        print(f"{k[0]:34s} {k[1]:5s} {worst[k]:.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
