cd "$(dirname "$0")/.."; export TMPDIR=/tmp; O=tools/tmp/r6s; mkdir -p $O; rm -rf /tmp/pf
U2PL_GRAPHS=0 U2PL_NO_SIDE_STREAM=1 U2PL_NO_WGRAD_STREAM=1 timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pf -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-direct-leg --no-config5-leg > $O/bench.json 2> $O/bench.err
f=$(find /tmp/pf -name '*kernel_stats.csv' | head -1); cp "$f" $O/serial_kernel_stats.csv; echo rc $?
