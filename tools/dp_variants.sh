log=$(mktemp)
for v in "A,B2,C0,C1,C2" "B2,C0,C1,C2" "C0,C1,C2" "none"; do
  TNT_DP_EAGER=$v timeout -k 10 200 python bench.py --force-dp --full --no-cpu-baseline --no-config3 --steps 300 --warmup 30 > "$log" 2>&1 \
    || { rc=$?; echo "$v: bench.py exited $rc"; tail -5 "$log"; break; }
  python - "$log" <<PY
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d=json.loads(l); print("$v", d["ms_per_step"], d["config"]["step_ms_p10_p50_p90"])
PY
done
rm -f "$log"
