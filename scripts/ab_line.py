"""One line per bench.py --full result file: value, value_unprofiled and the per-kernel ms per step.   usage: ab_line.py <result.json> <name>"""
import json
import sys

d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
k = d["roofline"]["kernel_ms_per_step"]
print(sys.argv[2], d["value"], d["value_unprofiled"], " ".join("%s=%.4f" % (a.replace("_kernel", ""), b) for a, b in k.items()))
