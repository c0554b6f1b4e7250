// Stand-in for <opencv2/features2d.hpp>: the reference includes it and uses nothing from it.
