#!/bin/bash
# The A/B of the RSA signer's window width and block size (DESIGN.md K19,
# profiles/r23_rsa_sign.json "ab"): variants of libcordahip.so that differ in rsa.hip's
# object alone, each measured by tools/rsa_sign_bench.py --sign-only, one process a
# variant, the variants in turn, ROUNDS rounds in one job.
#   tools/rsa_sign_ab.sh build          where hipcc is (no GPU needed): ab_libs/<tag>/libcordahip.so
#   tools/rsa_sign_ab.sh run [outdir]   on the GPU: <outdir>/<tag>_r<round>.json and <outdir>/ab.json
# VARIANTS: "tag:window:block" entries; the shipped build is measured beside them as "shipped".
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
VARIANTS=${VARIANTS:-"w3:3:64 w4:4:64 w5:5:64 w4b128:4:128 w3b128:3:128"}
ROUNDS=${ROUNDS:-2}
case "$1" in
build)
  make -s -j8 -C "$R/corda_amd/csrc"  # the main build's objects: every unit but rsa.hip's is reused
  for v in $VARIANTS; do
    IFS=: read tag win blk <<< "$v"
    mkdir -p "$R/ab_libs/$tag" "$R/build/ab/$tag"
    cp -p "$R"/build/obj/*.o "$R/build/ab/$tag/"
    rm -f "$R/build/ab/$tag/rsa.o"
    make -s -C "$R/corda_amd/csrc" OUT="$R/ab_libs/$tag/libcordahip.so" OBJDIR="$R/build/ab/$tag" \
      PROBE="$R/ab_libs/$tag/libcordaprobe.so" \
      EXTRA_FLAGS="-DCORDAHIP_RSA_SIGN_WIN=$win -DCORDAHIP_RSA_SIGN_BLOCK=$blk"
    # what the compiler made of the three signing kernels (registers, scratch, occupancy, LDS)
    (cd "$R/corda_amd/csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} -O3 -std=c++17 -fPIC --offload-arch=gfx950 \
      -DCORDAHIP_RSA_SIGN_WIN=$win -DCORDAHIP_RSA_SIGN_BLOCK=$blk -Rpass-analysis=kernel-resource-usage \
      -c -o /dev/null rsa.hip 2>&1 | awk '/Function Name/ { f = /rsa_sign_keyed_kernel/ } f' |
      grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size" > "$R/ab_libs/$tag/resource_usage.txt") || true
    ls -la "$R/ab_libs/$tag/libcordahip.so"
  done
  ;;
run)
  out=${2:-$R/out/rsa_sign_ab}
  mkdir -p "$out"
  win0=$(sed -n 's/^#define CORDAHIP_RSA_SIGN_WIN \([0-9]*\)$/\1/p' "$R/corda_amd/csrc/rsa_sign.hpp")
  for round in $(seq 1 "$ROUNDS"); do
    for v in "shipped:$win0:" $VARIANTS; do
      IFS=: read tag win blk <<< "$v"
      lib=""
      [ "$tag" = shipped ] || lib="--lib $R/ab_libs/$tag/libcordahip.so"
      timeout -k 10 300 python "$R/tools/rsa_sign_bench.py" --sign-only --legs 2048 3072 4096 --steps 3 --warmup 1 \
        --variant "$tag" --window "$win" $lib --out "$out/${tag}_r$round.json" > "$out/${tag}_r$round.log" 2>&1
    done
  done
  python - "$out" <<'PY'
import glob, json, os, sys
out = sys.argv[1]
runs = []
for f in sorted(glob.glob(os.path.join(out, "*_r[0-9]*.json"))):
    r = json.load(open(f))
    runs.append({"variant": r["variant"], "window": r["window"], "round": int(f.rsplit("_r", 1)[1].split(".")[0]),
                 "legs": [{k: l[k] for k in ("leg", "mod_words", "sign_ms", "sign_ms_min", "sign_ms_max", "sign_per_s",
                                             "rejected")} for l in r["legs"]]})
json.dump({"runs": runs}, open(os.path.join(out, "ab.json"), "w"), indent=1)
for r in runs:
    print(r["variant"], "round", r["round"], [(l["mod_words"], round(l["sign_ms"], 1)) for l in r["legs"]])
PY
  ;;
*)
  echo "usage: $0 build | run [outdir]" >&2
  exit 2
  ;;
esac
