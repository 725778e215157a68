#!/usr/bin/env python3
"""`valu_rate xchg`'s JSON lines -> profiles/lane_exchange_rate.json: SIMD cycles per lane exchange by waves per SIMD, alone and
on top of a stream of independent v_fma_f32 (8 or 16 per exchange).
usage: summarize_lane_exchange.py profiles/lane_exchange_rate.txt profiles/lane_exchange_rate.json"""
import json
import sys

rows = [json.loads(l) for l in open(sys.argv[1]) if l.startswith("{")]
fma = {r["waves_per_simd_launched"]: r["simd_cycles_per_fma_from_wall"] for r in rows if r["instr"] == "v_fma_f32"}
out = {"_source": "tools/micro/valu_rate.hip xchg on 1x MI355X: cycles one SIMD needs per exchange unit, from the launch's wall time x "
                  "the measured clock; alone_by_waves: the unit back to back; over_fma_at_N_waves: the unit's time on top of 8 / 16 "
                  "independent v_fma_f32 per unit (a cost that blocks the SIMD stays, a latency private to the wave hides)",
       "v_fma_f32_by_waves": fma, "_rows": rows}
for name in sorted({r["instr"] for r in rows} - {"v_fma_f32"}):
    mine = [r for r in rows if r["instr"] == name]
    d = {"alone_by_waves": {str(r["waves_per_simd_launched"]): r["simd_cycles_per_unit_from_wall"] for r in mine if r["fma_per_exchange"] == 0}}
    for k in sorted({r["waves_per_simd_launched"] for r in mine if r["fma_per_exchange"]}):
        d["over_fma_at_%d_waves" % k] = {"per_%d_fma" % r["fma_per_exchange"]: r["simd_cycles_per_exchange_over_fma"]
                                         for r in mine if r["fma_per_exchange"] and r["waves_per_simd_launched"] == k}
    out[name] = d
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "_rows"}, indent=1))
