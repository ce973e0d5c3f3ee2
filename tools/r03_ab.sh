# round-3 A/B driver: bash tools/r03_ab.sh <tag> [pytest args] -- runs tests + profiles, logs under $RESULTS_DIR/<tag>_* (default results/)
tag=${1:-ab}; shift
res=${RESULTS_DIR:-results}; mkdir -p "$res"   # every result of this script
python -m pytest ${*:-tests} -m gpu -x -q -s 2>&1 | tail -60 > "$res"/${tag}_tests.log
python tools/decoder_profile.py faces_objects 32 20 > "$res"/${tag}_decoder.txt 2>&1
python tools/decoder_profile.py flattened 16 20 > "$res"/${tag}_decoder2.txt 2>&1
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > "$res"/${tag}_bench.json 2> "$res"/${tag}_bench.err
tail -4 "$res"/${tag}_tests.log; grep median "$res"/${tag}_decoder*.txt; tail -3 "$res"/${tag}_bench.err; cut -c1-220 "$res"/${tag}_bench.json
