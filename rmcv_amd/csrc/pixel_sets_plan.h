// pixel_sets_plan.h -- the two pixel-output sets of a pipeline's hot context ("two pixel-output sets"): which set a batch takes
// and what its streams wait for.  Pure functions of plain values, beside batch_plan.h, so that a host compiler alone can check them
// (tests/test_pixel_sets_plan.py).
//
// A hot context meets a batch every `hot` calm batches.  With one set of what the pixel kernel writes (bit plane, row masks, byte image, image
// mask) that batch's pixel kernel waits for the sparse stage of the context's batch before: `hot` steps of slack, and the sparse stage's
// tail exceeds them a few times in a hundred.  With two sets taken in turn it waits for the batch before THAT -- the last one in the same
// set -- and the slack is doubled.  The sparse stage's tables stay one per context: the batch's sparse stream waits for the context's last
// batch instead, which costs nothing where both are on one stream.
#pragma once

#include <stdint.h>

namespace rmcv {

// the set a batch takes in context j = hot_seq % hot: the rotation's laps alternate.  Everything that is not `fast`, and every context
// without a second set (sets == 1), takes set 0.
inline int pixel_set_for(bool fast, uint64_t hot_seq, int hot, int sets)
{
    return fast && hot > 0 && sets > 1 ? (int)((hot_seq / (uint64_t)hot) & 1u) : 0;
}

// What the batch's streams wait for beyond the slot's own ev_done:
//   pixel_ctx_last  the pixel stream waits for the context's last batch (batch_plan.h: waits_for_free says at which event) -- the one wait
//                   there was with one set.  It stays for every batch that is not fast, for contexts without a second set, and wherever
//                   the binding enqueues work on the pixel stream: a changed geometry zeroes BOTH sets and the sparse stage's planes and
//                   recomputes the frame order, all of which the context's last batch may still read
//   pixel_set_last  otherwise: the pixel stream waits for the end of the last batch that used the same set of the context (an event of the
//                   set's own, recorded beside that batch's ev_done) ...
//   pixel_ctx_bin   ... and for the PIXEL kernel of the context's last batch (its ev_bin): the two share the context's strip queue.  Nothing
//                   to wait for where both are on one pixel stream (4 hot contexts over 2 pixel streams); with an odd `hot` they are not
//   sparse_ctx_last the batch's sparse stream waits for ev_done of the context's last batch in front of its sparse stage: the two share
//                   the context's one set of tables.  Always, whatever the batch is: every sparse stage of a context is then behind
//                   everything of the context's batches before, and a wait for the last one covers them all
struct SetWaits { bool pixel_ctx_last, pixel_set_last, pixel_ctx_bin, sparse_ctx_last; };
inline SetWaits pixel_set_waits(bool fast, int sets, bool bind_enqueues)
{
    const bool old = !fast || sets < 2 || bind_enqueues;
    return {old, !old, !old, true};
}

} // namespace rmcv
