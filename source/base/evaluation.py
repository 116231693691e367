from ppsurf_amd.evaluation import make_quantitative_comparison, write_metric_table  # noqa: F401
