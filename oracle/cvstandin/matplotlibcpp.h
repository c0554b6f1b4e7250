// Stand-in for matplotlibcpp.h: the reference includes it and uses nothing from it.
