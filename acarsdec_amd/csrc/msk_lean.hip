// msk_lean.hip -- the demodulator of msk.hip with the framing state machine taken OFF the per-bit path (round 6).
//
// msk_demod_kernel (msk.hip) runs putbit() / decodeAcars() after every bit decision: ~55 of the ~325 instructions a wave
// issues per bit period, on a loop that is bound by the number of instructions it issues.  The PLL does not need the
// framing result -- except when decodeAcars() resets the loop (`MskDf = 0`, acars.c:242).  This kernel therefore runs the
// bit periods in SEGMENTS of up to 8 bits: inside a segment a period only keeps what framing will need (the sign of the
// soft symbol under both polarities -- two 1-bit shift registers --, the level sum, the sample index), and after the
// segment the framing of its bits is done at once:
//   * hunting for sync (acars.c:252-265): all window positions of the segment compared with SYN and ~SYN bit-parallel,
//   * text (acars.c:303-341): a segment of <= 8 bits closes at most one byte,
//   * everything else through decode_acars() (msk_common.h), the same function msk.hip calls, on a rare branch.
// Exactness: a segment ends BEFORE any bit at which the reference could reset the loop.  Such a bit is always the closing
// bit of a byte in one of the states SYN2, SOH1, END, CRC2 (kept inline for its sample stamp) or TXT next to its
// error / length limits, and how many bits away that is (nbits) is known when the segment starts; from WSYN, TXT or
// CRC1 the next such bit is at least 8 bits behind the next byte boundary.  The closing bit itself is processed the way
// msk.hip does it (framing inline, between the bit decision and the loop filter, msk.c:122-130).  Same operations in the
// same order per channel as msk.hip and the reference; tests compare state, blocks and text of both kernels bit for bit.
//
// Used for every in_callback-shaped launch, with or without a bit log (with ACG_F_BITLOG the segment's per-bit records are made
// under the polarity of MskS + k and turned on the rare branch that finds a ~SYN in front of them): 16-byte aligned dm rows,
// len % 32 == 0, not the precise-mixer mode, 4 or 8 lanes per channel (ACG_MSK_LEAN4=0 keeps msk.hip's kernel for 4);
// ACG_MSK_NOLEAN=1 (tuning table) keeps msk.hip's kernel for same-process A/B.
//
// Issue order of a period (round 7).  One wave per SIMD runs this loop, so an LDS round trip that the period's own instructions do
// not cover is paid in full on the chain that sets the bit rate.  front() therefore issues, pinned with two sched_barriers:
//   sin/cos table address and read -> tap phase o -> h[o + 12 j] and the five old ring entries (reads) | the mixer's series and
//   rotation -> ring write -> the six newest ring entries (reads) | the five old taps' arithmetic -> wave-wide test -> decide(),
//   which only consumes what front() read,
// and "every lane fired, the segment goes on" is laid out as the fall-through.  One wave's LDS operations execute in order, so the
// newest-tap reads see the ring write in front of them; every wait is a counted one that leaves the younger reads in flight
// (which needs every scalar load retired before the loop: see where the epilogue's arguments are loaded).
// Same operations on the same operands as before.  Each step was timed against the order before it (newest-tap reads in decide(),
// no barrier in front of the mixer, table read inside the mixer, the compiler's block order), and two more steps were measured and
// not taken (1 / s started where df is set; the branch hint on `quick` as well): DESIGN 4, which also names the revision from
// which profiles/probe/build_ab.py builds those arms again.
// tests/test_lean_issue_order.py pins the order in the assembly.
//
// The front of a period (round 8).  A period takes up to six samples, each a VCO phase step (add, compare with 2 pi, select, fma) and
// a clock step (widen, add, narrow); the two chains only share the step s.  The compiler's order ran them one behind the other:
// clock steps 1-4, the test on `quick`, then phase steps 2-6 and clock steps 5 and 6 under the branch (machine sinking moves what is
// only used there), the sixth clock step in an exec-save block of its own, and behind the join the twelve selects with which a lane
// picks its own sample's phase.  front() now computes all six steps of both chains in ONE block in front of the test, side by side:
// steps 5 and 6 uncommitted (for a lane that is not `quick`, has fired or has no sample left they are arithmetic on registers whose
// result is dropped), the lane's pick issued behind the step that produces it, and the guarded block left with the commits (cnt, p,
// L.clk, fired: the same compares on the same values).  What keeps steps 1-4 in front of the branch is that steps 5 and 6 and the
// picks use them there; steps 5 and 6 are held by an empty asm volatile each (LEAN_HOLD_STEP), without which the sixth sinks again.
// Same operations on the same operands; a pick that a lane does not need (sample u >= cnt) goes to the ring's spare row as before.
// Switches (kept: the layout test compiles the old order to show that its first condition can fail): ACG_LEAN_AB_SPEC0 (steps 5 and
// 6 under the branch; steps 1-4 then carry a hold each, without which steps 2-4 sink behind it), ACG_LEAN_AB_PICK0 (the picks in the
// guarded block), ACG_LEAN_AB_VCO0 (with both of those: no hold on steps 1-4 either, which is the order before round 8).  Measured
// and not taken: a hold behind every step (1 % slower than holds on 5 and 6 only), the six newest taps as plain f32 (4 % slower), and
// the one-sample case by selects too; DESIGN 4.
// tests/test_lean_chain_layout.py pins the placement in the assembly.
//
// Where the bit records leave (round 9).  Every lane of a channel's group computes the identical record {soft symbol, level} of a
// period, and every period used to store it: a global_store_dwordx2 of all 64 lanes -- 64 addresses and 64 records out of the
// register file for 8 (or 16) distinct records -- issued by the one wave of its SIMD, so paid in full on the chain that sets the bit
// rate (the log cost 3.2 % of the kernel, alone on the chip exactly as beside the down-converter).  Now lane g of the group KEEPS
// records g, g + LPC, ... of the segment (two selects a period, on the lane masks the phase pick already has), the ~SYN branch
// turns the kept records in registers instead of reading them back from memory, and ONE store per lane (two with 4 lanes per
// channel) behind the segment's framing writes them: the same values at the same places.  The period that closes a segment
// msk.hip's way stores its own record as before.  Measured and not taken: the segment's text byte parked until behind the next
// refill's loads (the refill's `s_waitcnt vmcnt(0)` also waits for younger stores) -- nil.  ACG_LEAN_AB_REC0 is the order before;
// tests/test_lean_record_store.py pins the periods free of stores and compiles that switch to show the condition can fail.
//
// Slots that carry no arithmetic (round 10).  The period is paced by the number of slots it issues, and a wait, a no-operation or a
// register copy takes one: two `s_nop 0` MORE in front() cost 0.24 % of the kernel.  Eight came out of a period's 262: the
// compiler's three counted waits in front of the five old taps (lgkmcnt 9, 8, 7: for reads a whole sin/cos series old) are ONE,
// pinned behind the newest-tap reads (left free, the scheduler moves it behind the taps and the three come back); the hold of step 5
// leaves the clock out, so the fifth clock step fills the two slots that were `s_nop 0` in front of the phase picks; and the
// mixer's Horner steps that add a constant held in registers are three-address fmas (sincos_tab_rotate3, msk_common.h: left to the
// compiler, v_mov_b64 + v_fmac_f64 each).  Same operations on the same operands.  Measured and not taken: one wait in front of the
// six newest taps (they are not back yet: 0.7 % slower), the odd old taps' h[] half picked by op_sel in an asm (two copies fewer,
// 0.25 % slower), x - 3 pi / 2 with the constant negated in the operand and the segment's bit count set where a period leaves it
// (both longer, the second by 50 registers: not run), and a prologue that issues all its loads in one block, no branch around
// any of them (one round trip to memory instead of four in front of the loop: nil on the trace).  ACG_LEAN_AB_WAIT0 / _NOP0 / _HORN0 are the orders before;
// tests/test_lean_slots.py pins the counts and compiles those switches to show that its bounds can fail.  DESIGN 4.
//
// The closes that end a segment (round 11).  On the bench's traffic a wave gets 6.9 periods per segment, not 8: one period in 22
// closes a segment msk.hip's way, and in four cases out of five the channel that forces it stands in SYN2 behind a false sync
// (profiles/probe/lean_segment_stats.py).  frame_bit<true>() (msk_common.h) applies the closes in SYN2, SOH1-without-SOH and END by
// selects (here only: msk.hip frames after every bit, where the selects cost more than the walk saves), so that the closing period enters decode_acars() only for a sync, a SOH, a text byte that is not plain and the CRC bytes:
// 68 instructions and 4 of 26 branches fewer laid out in that period.  ACG_LEAN_AB_CLOSE0 is the text before;
// tests/test_lean_exits.py pins the figures and compiles the switch to show they can fail.  The periods of the segment are untouched.
// Built and not taken: lvk[] / nk[] without their zero fill, which is what the per-exit copy blocks behind the unrolled loop mostly
// write (both: one or two taken branches per exit, but a register copy MORE in each of periods 3-8, over test_lean_slots.py's
// bound; lvk[] alone: the periods hold, the copy blocks halve, worth ~0.1 % by the price of a slot: not run).  profiles/LEDGER.md, round 11.
//
// Fewer channels per wave (round 12).  A cut is wave-wide, so what the cuts cost falls with the channels per wave, and at 1024
// channels the 8-lane kernel fills 128 of the chip's 1024 SIMDs.  The kernel's text is in msk_lean_kernel.h; this file keeps its eight
// instantiations (4 and 8 lanes, both workgroup shapes: their assembly is what it was, line for line) and msk_lean_wide.hip
// instantiates 16 lanes per channel for four-wave workgroups: the default up to 1024 channels (acg_create), 0.944 -> 0.911 ms per call
// alone and the headline step -3.1 %.  A period's text does not depend on the width (tests/test_lean_wide_asm.py holds the wide
// kernels to the bounds pinned here).  profiles/LEDGER.md, round 12.
//
// What this kernel shares with msk.hip -- the state's way in and out, the LDS layout, the phase detector, the loop filter, the inline
// framing step of the closing period -- is in msk_common.h; the dm window's two lambdas are msk.hip's, spelled out here as there.
#include <hip/hip_runtime.h>
#include "acg_internal.h"

#include "msk_common.h"

#include "msk_lean_kernel.h"

// msk.hip's launcher hands over here when the launch qualifies (see the head of this file)
extern "C" int acg_launch_msk_lean(const MskArgs* a, int lpc, int wpg, unsigned int grid, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(64 * wpg);
#define LEAN_LAUNCH(L_, W_) do { if (a->bits) hipLaunchKernelGGL((msk_lean_kernel<L_, W_, true>), dim3(grid), blk, 0, s, *a); \
                                 else hipLaunchKernelGGL((msk_lean_kernel<L_, W_, false>), dim3(grid), blk, 0, s, *a); } while (0)
    switch (lpc * 16 + wpg) {
    case 4 * 16 + 1: LEAN_LAUNCH(4, 1); break;
    case 8 * 16 + 1: LEAN_LAUNCH(8, 1); break;
    case 4 * 16 + 4: LEAN_LAUNCH(4, 4); break;
    case 8 * 16 + 4: LEAN_LAUNCH(8, 4); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef LEAN_LAUNCH
    return (int)hipGetLastError();
}
