"""rustybam_amd -- MI355X (gfx950) CIGAR-walk engine behind rustybam's liftover / break-paf / stats path.

The product is the C-ABI shared library ``librustybam_amd.so`` (include/rustybam_amd.h) built from
``rustybam_amd/csrc``.  This Python package is only the ctypes plumbing used by tests and bench.py;
it never falls back to a CPU implementation: if the library or a gfx950 device is missing, calls
raise.
"""
from .capi import (Engine, RbError, lib, lib_path, HIT_DT, NORM_DT, REDUCE_DT, COUNTERS_DT, PAIR_DT, PIECES_INFO_DT,  # noqa: F401
                   BSEARCH_MODERN, BSEARCH_LEGACY, LIFT_EARLY_EXIT, LIFT_DESCRIPTORS, LIFT_FUSED_SCAN, LIFT_OP_STARTS, BREAK_ONE_WALK, TRIM_IN_PLACE, HIT_INSIDE, HIT_GENERIC, HIT_DESCRIPTOR, NF_COVERED, RD_OK, RD_FILTERED, RD_BAD_CIGAR, RD_SEQ_SHORT, exported_symbols, declared_symbols,
                   PAIRS_INFO_DT, PAIRS_ORIENT, PAIRS_FILTER, PAIRS_DECL_PANIC, PAIRS_DECL_KEY, PAIRS_DECL_WRAP, PAIRS_DECL_ZERO_SPAN, pairs_shape, host_pairs_rows,
                   pairs_records_shape, host_pairs_records,
                   ALN_DT, MD_OK, MD_UNUSUAL, ALN_OK, ALN_PANIC_DEL_FIRST, ALN_PANIC_HARDCLIP, ALN_PANIC_NONE, ALN_PANIC_MD_ASSERT, ALN_MD_STATUS, ALN_WARN_M, md_shape,
                   BAM_OK, BAM_SHORT_BLOCK, BAM_NO_FIT, BAM_BAD_NAME, bam_shape, bam_reads_shape,
                   NFT_FULL, NFT_SMALL, nucfreq_text_shape)
