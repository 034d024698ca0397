/* track_ref_hypot.h -- force-included (cc -include) in front of oracle/rmcv_oracle_track.c by tests/track_ref.py: the effect of
 * -Dhypot=trk_ref_hypot, which glibc's <math.h> does not survive on the command line (its prototypes are built by pasting the
 * function's name).  <math.h> is read first, under its own names; the oracle's later #include of it is a no-op. */
#include <math.h>
double trk_ref_hypot(double x, double y);
#define hypot trk_ref_hypot
