from ppsurf_amd.comparison import parse_arguments, comparison_rec_mesh_template, main  # noqa: F401

if __name__ == '__main__':
    main()
