set -o pipefail
mkdir -p bench_out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > bench_out/gpu_tests.log 2>&1 && \
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/smoke.log 2>&1 && \
timeout -k 10 300 python bench.py --full > bench_out/bench_default.json 2> bench_out/bench_default.err && \
timeout -k 10 300 python bench.py --full --config C3 --steps 200 --warmup 20 > bench_out/bench_C3.json 2> bench_out/bench_C3.err && \
timeout -k 10 300 python bench.py --full --config C4 --steps 100 --warmup 20 > bench_out/bench_C4.json 2> bench_out/bench_C4.err
