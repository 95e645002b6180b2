"""atsc_amd -- MI355X-native ATSC compression core (per-frame auto-compressor path).

The product is libatsc_hip.so (hand-written gfx950 kernels behind the C ABI in
include/atsc_hip.h).  This package only loads it and moves pointers around."""
from . import capi  # noqa: F401
from .capi import AUTO, CONSTANT, FFT, IDW, NOOP, POLYNOMIAL, RLE, AtscError  # noqa: F401
from .capi import QUANTILE_HIGHER, QUANTILE_LINEAR, QUANTILE_LOWER, QUANTILE_NEAREST  # noqa: F401
from .capi import HIST_LEFT_CLOSED, HIST_MAX_EDGES, HIST_RIGHT_CLOSED  # noqa: F401
from .capi import RUNS_EQ, RUNS_GE, RUNS_GT, RUNS_LE, RUNS_LT, RUNS_NE, RUNS_NONE  # noqa: F401
from .capi import EXTREMES_MAX_K, EXTREMES_NONE  # noqa: F401
from .engine import EXTREME, extremes_merge, window_extremes_dtype  # noqa: F401
from .stream import extremes_data_windows  # noqa: F401
from .capi import VALUES_MAX_K  # noqa: F401
from .engine import VALUE_COUNT, VALUE_MODE, values_merge, values_mode, window_values_dtype  # noqa: F401
from .stream import values_data_windows  # noqa: F401
from .engine import SELECTED, select_bytes  # noqa: F401
from .capi import ROLLING_MAX_WIDTH  # noqa: F401
from .engine import WINDOW_ROLLING, rolling_offsets, rolling_outputs  # noqa: F401
from .stream import rolling_data_windows, rolling_delta_data_windows, rolling_moments_data_windows  # noqa: F401
from .stream import rolling_pair_data_windows, rolling_runs_data_windows  # noqa: F401
from .capi import ROLLING_QUANTILE_MAX_WIDTH  # noqa: F401
from .stream import rolling_quantile_data_windows  # noqa: F401
from .stream import rolling_histogram_data_windows  # noqa: F401
from .capi import ACROSS_MAX_STREAMS  # noqa: F401
from .engine import ACROSS_RECORD, across_offsets, across_outputs  # noqa: F401
from .stream import across_data_windows, across_extremes_data_windows, across_quantile_data_windows  # noqa: F401
from .engine import ACROSS_FIT, ACROSS_MOMENTS, across_moments_fit, across_moments_merge  # noqa: F401
from .stream import across_moments_data_windows  # noqa: F401
from .stream import across_histogram_data_windows  # noqa: F401
from .stream import across_values_data_windows  # noqa: F401
from .engine import WINDOW_PAIR, WINDOW_PAIR_FIT, pair_fit  # noqa: F401
from .engine import pair_matrix_correlation, pair_matrix_index, pair_matrix_records  # noqa: F401
from .stream import pair_matrix_data_windows  # noqa: F401
from .stream import select_data_windows  # noqa: F401
from .engine import (WINDOW_DELTA, WINDOW_DELTA_FIT, WINDOW_FIT, WINDOW_MOMENTS, WINDOW_RUNS, WINDOW_STATS, Context, DPlan, Plan,  # noqa: F401
                     bro_find_window, bro_open, bro_prefix, bucket_windows, chunk_sizes, clean_data, delta_derive,
                     histogram_edges_uniform, moments_fit, runs_merge)
from .stream import (CompressedStream, aggregate_data_windows, bro_read_file, compress_data, csv_read,  # noqa: F401
                     decompress_data, decompress_data_window, delta_data_windows, histogram_data_windows,
                     moments_data_windows,
                     quantile_data_windows, runs_data_windows,
                     wbro_from_bytes, wbro_read, wbro_to_bytes, wbro_write)
from .vsri import Metric, Vsri, day_elapsed_seconds, read_samples_from_csv_file, write_samples_to_csv_file  # noqa: F401
