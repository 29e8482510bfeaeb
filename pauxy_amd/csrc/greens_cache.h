// What the Green's function buffers of a handle currently hold, and the per-launch request / result of an evaluation.
#pragma once

// The cached Green's function of the walk (afq_handle::gf).
//
// kept     what the last evaluation left for the CURRENT phi of every walker: nothing; FULL, the per-spin Ghalf with the
//          overlaps in ovlp_new (the end-of-step evaluation of afq_propagate_finish, or an energy update's own); SUM_ONLY,
//          the overlaps and the spin sum Ghalf_a + Ghalf_b (Hubbard: the diagonal sums) -- all the next step's force bias
//          reads -- after a step announced with afq_estimates_fuse_next, whose per-spin store was skipped.  Everything that
//          writes phi, psi or Ghalf drops it; what only reads takes it and puts it back.
// enabled  a handed-out device pointer turns the cache off for the life of the handle: the caller may write through it.
// version  bumped by every writer of Ghalf (and by whatever else makes a product derived from it stale: new walkers, new
//          half-rotated vectors).  The products are stamped with the version they were made from and are current while
//          the stamps match -- a bump makes all of them stale by construction:
//   gsum     ghalf_sum: written by the small Green's function kernel itself, else by ghalf_sum_kernel ahead of the force bias
//   gdiag    Hubbard: diag(G_s) as partial sums over row blocks, written by the Ghalf GEMM itself (k_bigdet.hip)
//   closed   this Ghalf comes from a launch that compared the spin blocks of EVERY walker (greens_small_kernel,
//            ghalf_closed_check_kernel, the unpack of a comb): while current, "*closed_bad < closed_epoch" ON THE DEVICE means
//            Ghalf_b == Ghalf_a for every walker, and the exchange energy evaluates one spin (k_energy.hip)
//   vbias    the force-bias partials in vbias (the Coulomb vectors of an energy evaluation are the next step's force
//            bias); a multi-determinant trial keeps one stamp per determinant (afq_handle::DetOps::vbias)
struct GreensCache {
    enum Kept { NOTHING, FULL, SUM_ONLY };
    enum Carry { SUM = 1, DIAG = 2, CLOSED = 4 };      // the stamps cloned() can take across its bump

    class Stamp {                                       // (0: never made)
        unsigned long long v = 0;
    public:
        bool current(const GreensCache &c) const { return v != 0 && v == c.version; }
        void mark(const GreensCache &c) { v = c.version; }
        void clear() { v = 0; }
    };

    Kept kept = NOTHING;
    bool enabled = true;
    unsigned long long version = 1;
    Stamp gsum, gdiag, closed, vbias;

    void drop() { kept = NOTHING; }
    void keep(Kept k) { kept = k; }                     // after an evaluation, or what take() returned
    Kept take() { const Kept k = kept; kept = NOTHING; return k; }
    void rewritten() { ++version; }
    // whole walkers were copied over others, their Ghalf with them: a new content, but the stamps named in carry (Carry
    // bits) hold for the copies as they held for the originals, provided they were current
    void cloned(int carry) {
        const bool s = (carry & SUM) && gsum.current(*this), d = (carry & DIAG) && gdiag.current(*this),
                   c = (carry & CLOSED) && closed.current(*this);
        ++version;
        if (s) gsum.mark(*this);
        if (d) gdiag.mark(*this);
        if (c) closed.mark(*this);
    }

    // An entry point that is read-only on the walk: takes what is kept on entry (so that nothing is kept while the call
    // works on the handle's buffers, or after it fails half way) and puts it back when told the whole call has succeeded.
    class ReadOnly {
        GreensCache *c; Kept was;
    public:
        explicit ReadOnly(GreensCache *c_) : c(c_), was(c_ ? c_->take() : NOTHING) {}
        void succeeded() { if (c) c->keep(was); }
    };

    // An evaluation into buffers that are not the walk's (a window's own Ghalf): on the way out the version and the
    // closed-shell verdict are back where they were, and with them everything contracted from the walk's cached Ghalf.
    class Foreign {
        GreensCache &c; unsigned long long version; Stamp closed;
    public:
        explicit Foreign(GreensCache &c_) : c(c_), version(c_.version), closed(c_.closed) {}
        ~Foreign() { c.version = version; c.closed = closed; }
        Foreign(const Foreign &) = delete;
        Foreign &operator=(const Foreign &) = delete;
    };
};

// What the caller of one Green's function / overlap evaluation asks of the launch, and what the launch did about it.
struct GreensRequest {
    bool ride_weight = false;       // the step's weight update may ride on the determinant kernel ...
    double2 eshift = {0.0, 0.0};    // ... with this energy shift
    bool may_skip_store = false;    // nobody will read the per-spin Ghalf: spin sum / diagonal sums only, where a kernel can
    double2 *det_a = nullptr;       // where the alpha determinants go (multi-determinant trials), or null
};
struct GreensResult {
    bool weight_rode = false;       // the weight update is done
    bool store_skipped = false;     // the per-spin Ghalf was not written
};
