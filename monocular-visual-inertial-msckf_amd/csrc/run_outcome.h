// The outcome of an update, decided from its status words ("Status words").  Host code without a HIP header:
// tests/test_run_outcome.py compiles it with the host compiler and checks every row of the table.
#pragma once

enum class Outcome { Ok, Noop, NotSpd, Timeout, Unwritten, Overflow };

// gain: K6-K7 ran (else no status word is this run's).  word1_ours / word4_ours: a launch of this run wrote status word 1 / 4
// (nothing resets them between runs: a word that is not ours is stale and is not read).  n_accepted: features that passed the gate.
// status: 0 ok, 1 a pivot was not a positive normal number, 2 a launch gave up waiting, 3 the word's mirror in host memory was
// never written; word 4 bit 1: the split records held more remainder rows than the merge takes.
inline Outcome decode_outcome(bool gain, bool word1_ours, bool word4_ours, int n_accepted, const int status[5]) {
    if (n_accepted <= 0) return Outcome::Noop;
    if (!gain) return Outcome::Ok;
    const int s0 = status[0], s1 = word1_ours ? status[1] : 0;
    if (s0 == 3 || s1 == 3) return Outcome::Unwritten;
    if (s0 == 2 || s1 == 2) return Outcome::Timeout;
    if (s0 != 0 || s1 != 0) return Outcome::NotSpd;
    if (word4_ours && (status[4] & 2)) return Outcome::Overflow;
    return Outcome::Ok;
}
