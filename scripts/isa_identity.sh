#!/usr/bin/env bash
# Refactor check for the kernel directory: every .hip file must compile to the device assembly it compiled to at <parent-rev>.
#   scripts/isa_identity.sh <parent-rev> [file.hip ...]      (no files given: every .hip in analysisgnn_amd/csrc)
# The parent's copy of each file is compiled next to the parent's headers, both sides with the Makefile's flags plus
# --cuda-device-only -S; comment-only lines, .file / .ident and the per-compilation __hip_cuid_<hash> symbol are normalised away
# (the recipe of profiles/relt_isa_identity.md).  Prints IDENTICAL or the first differing hunk per file; needs no GPU.
set -u
[ $# -ge 1 ] || { echo "usage: $0 <parent-rev> [file.hip ...]" >&2; exit 2; }
parent=$1; shift
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel) || exit 2
cd "$root" || exit 2
csrc=analysisgnn_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
JOBS=${JOBS:-8}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=$ARCH -Wall -Wno-unused-result --cuda-device-only -S"

if [ $# -eq 0 ]; then set -- "$csrc"/*.hip; fi
tmp=$(mktemp -d) || exit 2
trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/parent/$csrc" "$tmp/parent/include" "$tmp/out"
for h in $(git ls-tree --name-only "$parent" "$csrc/" include/ | grep -E '\.h$'); do
  git show "$parent:$h" > "$tmp/parent/$h" || exit 2
done

norm() { grep -vE '^\s*;' "$1" | grep -vE '^\s*\.(file|ident)' | sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g'; }

check_one() {
  local f=$1 name
  name=$(basename "$f")
  if ! git show "$parent:$csrc/$name" > "$tmp/parent/$csrc/$name" 2>/dev/null; then
    echo "$name: NEW (not in $parent)" > "$tmp/out/$name.txt"; return 1
  fi
  if ! $HIPCC $FLAGS -I "$tmp/parent/include" "$tmp/parent/$csrc/$name" -o "$tmp/out/$name.parent.s" 2> "$tmp/out/$name.err" ||
     ! $HIPCC $FLAGS -I include "$csrc/$name" -o "$tmp/out/$name.new.s" 2>> "$tmp/out/$name.err"; then
    { echo "$name: COMPILE FAILED"; head -20 "$tmp/out/$name.err"; } > "$tmp/out/$name.txt"; return 1
  fi
  norm "$tmp/out/$name.parent.s" > "$tmp/out/$name.parent.norm"
  norm "$tmp/out/$name.new.s" > "$tmp/out/$name.new.norm"
  if diff "$tmp/out/$name.parent.norm" "$tmp/out/$name.new.norm" > "$tmp/out/$name.diff"; then
    echo "$name: IDENTICAL ($(wc -l < "$tmp/out/$name.new.norm") lines)" > "$tmp/out/$name.txt"; return 0
  fi
  # first hunk only: up to the second line that opens a hunk
  { echo "$name: DIFFERS"; awk '/^[0-9]/ { if (++n > 1) exit } { print "    " $0 }' "$tmp/out/$name.diff" | head -40; } > "$tmp/out/$name.txt"
  return 1
}

running=0
for f in "$@"; do
  check_one "$f" &
  running=$((running + 1))
  if [ "$running" -ge "$JOBS" ]; then wait -n; running=$((running - 1)); fi
done
wait

status=0
for f in "$@"; do
  name=$(basename "$f")
  cat "$tmp/out/$name.txt"
  grep -q ': IDENTICAL' "$tmp/out/$name.txt" || status=1
done
exit $status
