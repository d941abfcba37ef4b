"""The `cytospace` command line (cytospace/common/argument_parser.py): the reference's flags, short forms and defaults, with
two differences -- `-sm` offers SOLVER_METHODS and defaults to 'lapjv_hip' (main_cytospace here drives that solver only)."""
import argparse

from .linear_assignment_solvers import SOLVER_METHODS


def add_plotting_arguments(parser):
    parser.add_argument("-g", "--geometry", type=str, default="honeycomb",
                        help="spot layout of the ST data for plots: 'honeycomb' or 'square' (plots are not produced here)")
    parser.add_argument("-nc", "--num-column", type=int, default=3, help="columns of the figure grid (plots are not produced here)")
    parser.add_argument("-mp", "--max-num-cells-plot", type=int, default=50000,
                        help="most cells drawn in a single-cell plot (plots are not produced here)")


def build_parser():
    parser = argparse.ArgumentParser(
        prog="python -m cytospace_amd",
        description="CytoSPACE on AMD Instinct GPUs: assign single-cell transcriptomes to the spots of spatial transcriptomics "
                    "data by solving a linear assignment problem over a correlation-based cost.")
    required = parser.add_argument_group("Required arguments")
    required.add_argument("-sp", "--scRNA-path", type=str, default=None, required=True,
                          help="scRNA-seq counts: genes x cells table (.csv / .txt / .tsv) or a 10x matrix.mtx")
    required.add_argument("-ctp", "--cell-type-path", type=str, default=None, required=True,
                          help="cell type label of every scRNA-seq cell")

    parser.add_argument("-stp", "--st-path", type=str, default=None, help="ST counts: genes x spots")
    parser.add_argument("-cp", "--coordinates-path", type=str, default=None, help="coordinates of every ST spot")
    parser.add_argument("-srp", "--spaceranger-path", type=str, default=None,
                        help="Space Ranger tar.gz output (not supported here: pass -stp and -cp)")
    parser.add_argument("-stctp", "--st-cell-type-path", type=str, default=None,
                        help="cell type of every ST spot (single-cell ST data)")
    parser.add_argument("-ctfep", "--cell-type-fraction-estimation-path", type=str, default=None,
                        help="estimated cell type fractions of the ST sample (spot-resolution ST data)")
    parser.add_argument("-ncpsp", "--n-cells-per-spot-path", type=str, default=None,
                        help="number of cells in every ST spot (estimated from the ST counts when absent)")
    parser.add_argument("-o", "--output-folder", type=str, default="cytospace_results",
                        help="output folder, relative to the working directory")
    parser.add_argument("-op", "--output-prefix", type=str, default="", help="prefix of every output file name")

    parser.add_argument("-mcn", "--mean-cell-numbers", type=int, default=5,
                        help="mean number of cells per spot for the estimate: 5 suits Visium, about 20 legacy ST")
    parser.add_argument("--downsample-off", action="store_true", help="keep the scRNA-seq counts as they are")
    parser.add_argument("-smtpc", "--scRNA_max_transcripts_per_cell", type=int, default=1500,
                        help="cells with more transcripts are downsampled to this many")
    parser.add_argument("-sc", "--single-cell", action="store_true", help="the ST data has single-cell resolution")
    parser.add_argument("-noss", "--number-of-selected-spots", type=int, default=10000,
                        help="spots per partition in single-cell mode")
    parser.add_argument("-sss", "--sampling-sub-spots", action="store_true",
                        help="split the spots' cell slots into sub-spot partitions solved one by one")
    parser.add_argument("-nosss", "--number-of-selected-sub-spots", type=int, default=10000,
                        help="cell slots per sub-spot partition")
    parser.add_argument("-nop", "--number-of-processors", type=int, default=4,
                        help="partitions in flight at once on each GPU")
    parser.add_argument("-sm", "--solver-method", default="lapjv_hip", choices=list(SOLVER_METHODS),
                        help="linear assignment solver; main_cytospace here runs 'lapjv_hip' (the default)")
    parser.add_argument("-dm", "--distance-metric", default="Pearson_correlation",
                        choices=["Pearson_correlation", "Spearman_correlation", "Euclidean"],
                        help="cost of assigning a cell to a spot")
    parser.add_argument("-sam", "--sampling-method", default="duplicates", choices=["duplicates", "place_holders"],
                        help="how missing cells of a type are made up: repeat cells or synthesise place-holders")
    parser.add_argument("-se", "--seed", type=int, default=1, help="seed of numpy's and Python's generators")
    parser.add_argument("-p", "--plot-off", action="store_true", help="do not plot (this package never plots)")
    add_plotting_arguments(parser)
    return parser


def argument_parser(argv=None):
    """Parse argv (default: sys.argv[1:]) into main_cytospace's keyword arguments."""
    return vars(build_parser().parse_args(argv))
