# One sha256 per device code object: the six production translation units (Makefile
# flags, N20FLAGS on ntm_n20.hip) and the single-TU diag, diag20, poison and
# -DNTM_RU_ONLY20 builds, each compiled to device assembly with the __hip_cuid_ lines
# (which differ between two compiles of one source) dropped.  CPU only.
#   bash tools/asm_digest.sh [unit ...]     ->  "<sha256>  <unit>" lines (default: all ten)
#   bash tools/asm_digest.sh --per-kernel [unit ...]
#                                           ->  "<sha256>  <unit>  <kernel symbol>" lines: one
#       digest per function of each unit, over the text from the symbol's label to its
#       .Lfunc_end (code and kernel descriptor), without the comments and with the
#       unit-wide counters taken out of its local labels (.LBB<i>_<n>, .Lfunc_end<i>,
#       .Lpost_getpc<n>, .Ltmp<n>), so a kernel's digest does not depend on which kernels
#       the unit holds before it.  Two trees agree on a kernel exactly when its lines
#       agree (diff the two outputs).
#   ASM_DIR=dir bash tools/asm_digest.sh    also keeps the assembly in dir/<unit>.s;
#       ASM_REUSE=1 hashes the dir/<unit>.s already there instead of compiling
set -e
PER=0
if [ "$1" = --per-kernel ]; then PER=1; shift; fi
cd "$(dirname "$0")/../mpc-ntm-control_amd"
H="/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function --cuda-device-only -S"
N20="-mllvm -amdgpu-use-amdgpu-trackers=1"
N20DEFS="-DNTM_N20_NO_RATE=1"    # the Makefile's N20DEFS (diag20); ntm_n20.hip sets it itself
DIAG="-DNTM_CH=5 -DNTM_CHUNK_UNROLL=2 -Wno-pass-failed -DNTM_STAMPS"
ONE="csrc/ntm_kernels.hip -DNTM_SINGLE_TU"
UNITS=${*:-ntm_kernels ntm_n20 ntm_n20near ntm_n20near1w ntm_n50 ntm_n50m3 diag diag20 poison ru_only20}
D=${ASM_DIR:-$(mktemp -d)}
mkdir -p "$D"
for n in $UNITS; do
  case $n in
    ntm_n20) F="$N20 csrc/$n.hip";;
    ntm_*) F="csrc/$n.hip";;
    diag) F="$DIAG $ONE";;
    diag20) F="$DIAG $N20 $N20DEFS $ONE";;
    poison) F="-DNTM_POISON=1e300 $ONE";;
    ru_only20) F="-DNTM_RU_ONLY20 $ONE";;
    *) echo "unknown unit $n" >&2; exit 1;;
  esac
  [ -n "$ASM_REUSE" ] && [ -s "$D/$n.s" ] && continue
  $H $F -o - | grep -v __hip_cuid_ > "$D/$n.s" &
done
wait
cd "$D"
for n in $UNITS; do
  test -s $n.s || { echo "$n: compile failed" >&2; exit 1; }
  if [ $PER = 0 ]; then
    sha256sum $n.s | sed 's/\.s$//'
  else
    awk -v unit=$n '
      /^\t\.type\t.*,@function/ { fn = 1 }
      fn && !insym && /^[A-Za-z_][^ \t]*:/ {
        sym = $1; sub(/:$/, "", sym); insym = 1; fn = 0
        cmd = "sha256sum | sed \"s/-\\$/" unit "  " sym "/\""
      }
      insym {
        line = $0
        sub(/[ \t]*;.*$/, "", line)
        gsub(/\.LBB[0-9]+_/, ".LBB_", line)
        gsub(/\.Lpost_getpc[0-9]+/, ".Lpost_getpc", line)
        gsub(/\.Ltmp[0-9]+/, ".Ltmp", line)
        gsub(/\.Lfunc_end[0-9]+/, ".Lfunc_end", line)
        if (line != "") print line | cmd
      }
      insym && /^\.Lfunc_end[0-9]+:/ { close(cmd); insym = 0 }
    ' $n.s
  fi
done
