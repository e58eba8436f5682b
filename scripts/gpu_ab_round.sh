#!/bin/bash
# Runs on the GPU box via gpurun: A/B of the prebuilt library variants (scripts/ab_variants.py --build, in the build
# container), installs the fastest exact candidate as the library, then bench + rocprofv3 kernel stats + GPU tests.
# Usage: scripts/gpu_ab_round.sh <tag>     (outputs under gpurun_out/<tag>/)
set -u
TAG="${1:-ab}"
R="${GRAFT_REPO_ROOT:-$(pwd)}"
OUT="$R/gpurun_out/$TAG"; mkdir -p "$OUT"
cd "$R"
echo "== A/B =="; timeout 300 python scripts/ab_variants.py 2>&1 | tee "$OUT/ab_variants.txt" | tail -40
cp gpurun_out/ab_variants.json "$OUT/" 2>/dev/null
PICK=$(python - <<'PY'
import json
try:
    r = json.load(open("gpurun_out/ab_variants.json"))
    c = {k.split("/")[1]: v for k, v in r.items() if k.startswith("bf16 4GiB/") and k.split("/")[1] in ("r01z", "new", "late", "wmask") and v["exact"]}
    best = min(c, key=lambda k: c[k]["ms"])
    # the default build stays unless something beats it by more than 1 %
    if "new" in c and c["new"]["ms"] <= 1.01 * c[best]["ms"]:
        best = "new"
    print(best)
except Exception:
    print("new")
PY
)
echo "picked: $PICK" | tee "$OUT/picked.txt"
if [ "$PICK" != "new" ]; then cp "zipnn_amd/libzipnn_hip_ab_$PICK.so" zipnn_amd/libzipnn_hip.so; fi
echo "== bench =="; timeout 300 python bench.py --full --steps 20 --warmup 2 2>"$OUT/bench.err" | tail -1 | tee "$OUT/bench.json"
echo "== rocprofv3 kernel stats =="
cd /tmp && export TMPDIR=/tmp
timeout 240 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o bench -- python "$R/bench.py" --full --steps 20 --warmup 2 --no-cpu-baseline > "$OUT/rocprof.log" 2>&1
tail -2 "$OUT/rocprof.log"
find "$OUT/prof" -name '*kernel_stats*' | head -1 | while read f; do cp "$f" "$OUT/kernel_stats.csv"; head -8 "$f"; done
find "$OUT/prof" -name '*kernel_trace*' -size +20M -delete 2>/dev/null
cd "$R"
echo "== pytest -m gpu =="; timeout 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -6 | tee "$OUT/pytest_gpu.log"
echo "== done =="
