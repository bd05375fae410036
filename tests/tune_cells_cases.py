"""dz_tune_cells, the scoring geometry of the tuners' entry points (include/diart_amd.h): which members every entry
reads — the lists of the header's comments, which tests/test_tune_cells_host.py pins — and descriptors with members
taken out."""
import ctypes as C

from diart_amd import _lib

SEQUENTIAL = ("file_row_off", "file_chunk_off", "step_rows", "mids", "mid_cell", "file_cell_off", "cell_dur", "cell_ref")
KERNEL = ("file_chunk_off", "row_off", "mids", "mid_cell", "file_cell_off", "cell_dur", "cell_ref")
TRACK_PAIR = ("mids", "mid_cell", "file_cell_off", "dur_prefix", "ref_prefix")
SHAPE = ("n_files", "total_rows")

# entry -> the members it reads: pointers, then scalars
READS = {
    "dz_tune_score": SEQUENTIAL + SHAPE + ("max_speakers", "collar"),
    "dz_tune_score_core": KERNEL + SHAPE + ("max_cells", "max_speakers", "collar"),
    "dz_tune_score_gpu": KERNEL + SHAPE + ("max_cells", "max_speakers", "collar"),
    "dz_tune_ident_score": SEQUENTIAL + ("cell_step",) + SHAPE + ("total_chunks", "max_speakers", "collar"),
    "dz_tune_ident_score_core": KERNEL + ("cell_step",) + SHAPE + ("total_chunks", "max_cells", "max_speakers", "collar"),
    "dz_tune_ident_score_gpu": KERNEL + ("cell_step",) + SHAPE + ("total_chunks", "max_cells", "max_speakers", "collar"),
    "dz_tune_track_score_dur": KERNEL + SHAPE + ("collar",),
    "dz_tune_vad_host": TRACK_PAIR + ("collar",),
    "dz_tune_vad_score": ("file_chunk_off", "row_off") + TRACK_PAIR + SHAPE + ("collar",),
}
POINTERS = _lib.TuneCells.POINTERS


def pointers_read(entry):
    return [m for m in READS[entry] if m in POINTERS]


def copy_of(cells, **members):
    """A copy of the descriptor with `members` set."""
    c = _lib.TuneCells.from_buffer_copy(cells)
    for name, value in members.items():
        setattr(c, name, value)
    return c


def only_what_it_reads(cells, entry):
    """A copy with every member `entry` does not read NULL or 0."""
    return copy_of(cells, **{name: None if name in POINTERS else 0 for name, _ in _lib.TuneCells._fields_
                             if name not in READS[entry]})


def filled(pointer, max_speakers=5):
    """A descriptor for the refusal tests of the device entries: every pointer `pointer`, one file of one step."""
    c = _lib.TuneCells()
    for name in POINTERS:
        setattr(c, name, pointer)
    c.n_files = c.total_rows = c.total_chunks = c.max_cells = 1
    c.max_speakers, c.collar = max_speakers, 0.05
    return c


ref = C.byref
