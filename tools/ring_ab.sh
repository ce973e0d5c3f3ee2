set -x
res=${RESULTS_DIR:-results}; mkdir -p "$res"   # every result of this script
python -m pytest tests/test_gpu_ops.py tests/test_gpu_encoders.py -m gpu -x -q 2>&1 | tail -5 > "$res"/ring_tests.log
for r in 2 3 4; do
  export TELL_GEMM_RING=$r
  python tools/bench_decoder_gemms.py > "$res"/ring${r}_decgemm.txt 2>&1
  python tools/bench_conv.py 32 > "$res"/ring${r}_conv.txt 2>&1
  python tools/decoder_profile.py faces_objects 32 20 > "$res"/ring${r}_decoder.txt 2>&1
  python tools/resnet_profile.py 32 20 > "$res"/ring${r}_resnet.txt 2>&1
done
for r in 2 4; do
  export TELL_GEMM_RING=$r
  python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary > "$res"/ring${r}_bench.json 2> "$res"/ring${r}_bench.err
done
tail -3 "$res"/ring_tests.log; tail -2 "$res"/ring*_decoder.txt "$res"/ring*_resnet.txt; cut -c1-200 "$res"/ring*_bench.json
