cd "$GRAFT_REPO_ROOT"
o=${1:-bench_out/all_configs}; mkdir -p $o
python bench.py --full --config cfg1 --steps 20 --warmup 5 --no-cpu-baseline > $o/cfg1.json 2>/dev/null; echo cfg1 done
python bench.py --full --config cfg3 --steps 10 --warmup 3 --no-cpu-baseline > $o/cfg3.json 2>/dev/null; echo cfg3 done
python bench.py --full --config cfg4 --global-batch 128 --steps 10 --warmup 3 --no-cpu-baseline > $o/cfg4.json 2>/dev/null; echo cfg4 done
python bench.py --full --config cfg4_bf16 --global-batch 128 --steps 10 --warmup 3 --no-cpu-baseline --path engine > $o/cfg4_bf16.json 2>/dev/null; echo cfg4_bf16 done
python bench.py --full --global-batch 512 --steps 10 --warmup 3 --no-cpu-baseline --path engine > $o/cfg2_b512.json 2>/dev/null
python bench.py --full --global-batch 256 --steps 10 --warmup 3 --no-cpu-baseline --path engine > $o/cfg2_b256.json 2>/dev/null
python - "$o" <<'PY'
import json, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    try:
        d = json.loads([l for l in open(f) if l.startswith("{")][0])
        print(f.split("/")[-1], round(d["ms_per_step"], 2), round(d["value"], 1), round(d["roofline"]["whole_step"]["frac"], 4), round(d["roofline"]["frac"], 4), d.get("module_path", {}).get("ms_per_step"))
    except Exception as e:
        print(f, "failed", e)
PY
