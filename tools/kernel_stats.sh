ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/ks -- python3 $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-ahds > /tmp/ks.log 2>&1
grep -h "gip_" /tmp/ks/*/*_kernel_stats.csv | sed 's/(.*)"/"/' | cut -c1-110
