#!/bin/bash
# Issue slots between the MFMAs of k_run's hot tile (the certified one-wave dueling tile): per stream segment the MFMAs, VALU
# instructions, s_nop, s_waitcnt, memory and LDS instructions, and the non-MFMA slots per MFMA.   tools/isa_slots.sh [0|1] [extra hipcc flags]
#   unit 0 = k_run<512, fixed, dueling, TRAIN 0> (configs[3]).  RL_SLOTS_SRC=<dir> takes rl_run.hip from another tree (tools/build_at_commit.sh
#   leaves the sources of a commit in /tmp/rl_src_<tag>/reinlife_amd/csrc).  The segments are cut at the tile's MFMA numbers: input layer
#   pass 0 / 1 (60 each), hidden layer pass 0 / 1 (48 each), head (24) -- a segment runs from its first MFMA to the next segment's first.
cd "$(dirname "$0")/.." || exit 1
u=${1:-0}; shift
src=${RL_SLOTS_SRC:-reinlife_amd/csrc}
out=/tmp/isa_slots_u$u.s
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function --cuda-device-only -DRL_RUN_UNIT=$u "$@" -S $src/rl_run.hip -o $out 2>/dev/null || exit 1
# the first TRAIN 0 instantiation of k_run in the unit: from its label to its .Lfunc_end
awk '/^_ZN[0-9A-Za-z_]*5k_runILi512ELb1ELi[0-9]+ELi0EEE[^:]*:/ && !f {f=1} f {print} f && /^\.Lfunc_end[0-9]+:/ {exit}' $out > /tmp/isa_slots_k$u.s
grep -E "^\s*; (NumVgprs|ScratchSize):" <(awk '/^_ZN[0-9A-Za-z_]*5k_runILi512ELb1ELi[0-9]+ELi0EEE[^:]*:/ && !f {f=1} f {print} f && /; ScratchSize/ {exit}' $out)
awk '/s_barrier/{b++} /v_mfma/{m++} /scratch_load/{printf "reload at line %d (after barrier #%d, %d MFMAs before it): %s\n", NR, b, m, $0}' /tmp/isa_slots_k$u.s
awk '
function flush() { if (seg) printf "%-32s %5d %5d %6d %9d %5d %4d %5d   %.1f\n", name[seg], M, V, N, W, G, D, O, (V + N + W + G + D + O) / M }
BEGIN { name[1] = "input layer, pass 0 (1-60)"; name[2] = "input layer, pass 1 (61-120)"; name[3] = "hidden layer, pass 0 (121-168)"; name[4] = "hidden layer, pass 1 (169-216)"; name[5] = "head (217-240)";
        first[1] = 1; first[2] = 61; first[3] = 121; first[4] = 169; first[5] = 217;
        printf "%-32s %5s %5s %6s %9s %5s %4s %5s   %s\n", "segment of the hot tile", "MFMA", "VALU", "s_nop", "s_waitcnt", "vmem", "ds", "other", "non-MFMA per MFMA" }
/^[ \t]*v_mfma/ { m++; for (s = 1; s <= 5; ++s) if (m == first[s]) { flush(); seg = s; M = V = N = W = G = D = O = 0 } if (seg) M++; if (m == 240) { flush(); seg = 0 } next }
!seg || /^[ \t]*(;|\.|$)/ || /^[.A-Za-z_0-9]+:/ { next }
/^[ \t]*s_nop/ { N++; next }
/^[ \t]*s_waitcnt/ { W++; next }
/^[ \t]*(global_|buffer_|scratch_|flat_)/ { G++; next }
/^[ \t]*ds_/ { D++; next }
/^[ \t]*v_/ { V++; next }
{ O++ }' /tmp/isa_slots_k$u.s
