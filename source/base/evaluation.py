from ppsurf_amd.evaluation import make_quantitative_comparison, write_metric_table  # noqa: F401
from ppsurf_amd.comparison import (assemble_quantitative_comparison, make_dataset_comparison, make_html_report,  # noqa: F401
                                   _drop_stats_rows)
