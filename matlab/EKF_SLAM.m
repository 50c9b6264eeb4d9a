classdef EKF_SLAM < handle
    % Drop-in for the reference's EKF_SLAM (known correspondence) over libekfslam (MEX -> C ABI -> HIP).
    % Same constructor, properties (x P Q s C Rc s_cost s_thresh landmark_list observed -- all assignable, as in
    % the reference, EKF_SLAM.m:5-22) and methods (predict, f, append, measure, plot); x, P, s live on the GPU and are
    % fetched / stored on access.
    % NOT RUN under MATLAB in this repository's image (no MATLAB there) -- see INTEGRATION.md.
    properties (Dependent)
        x; P; Q; s;
    end
    properties
        C = 0.2; Rc = [.01, 5]; s_cost = 1e-11; s_thresh = 1e9;
        landmark_list; observed;
    end
    properties (Access = protected)
        hnd;
        Qassigned = [];     % a Q the caller assigned; predict() recomputes Q (EKF_SLAM.m:43-44), which drops it
    end
    methods
        function h = EKF_SLAM(capacity)
            if nargin < 1, capacity = 1024; end
            h.hnd = ekfslam_mex('create', h.abiMode(), capacity);
        end
        function delete(h), ekfslam_mex('destroy', h.hnd); end
        function v = get.x(h), v = ekfslam_mex('get_x', h.hnd); end
        function v = get.P(h), v = ekfslam_mex('get_P', h.hnd); end
        function v = get.s(h), v = ekfslam_mex('get_s', h.hnd); end
        function v = get.Q(h)
            if isempty(h.Qassigned), v = ekfslam_mex('get_Q', h.hnd); else, v = h.Qassigned; end
        end
        % assignment: x first (it fixes the number of landmarks), then s / P of matching size
        function set.x(h, v), ekfslam_mex('set_x', h.hnd, double(v(:))); end
        function set.P(h, v), ekfslam_mex('set_P', h.hnd, double(v)); end
        function set.s(h, v), ekfslam_mex('set_s', h.hnd, double(v(:))); end
        function set.Q(h, v), h.Qassigned = v; end
        function pushParams(h)   % forward the (re-assignable) tunables before each call that uses them
            ekfslam_mex('set_params', h.hnd, h.C, double(h.Rc(:)), h.s_cost, h.s_thresh, 0);
        end
        function predict(h, u)
            h.pushParams(); h.Qassigned = [];
            ekfslam_mex('predict', h.hnd, double(u(:)));
        end
        function [x_new, F] = f(~, x, u), [x_new, F] = ekfslam_mex('f', [], double(x), double(u(:))); end
        function append(h, u, R, landmarkPos, signature)
            ekfslam_mex('append', h.hnd, double(u(:)), double(R), double(landmarkPos(:)), double(signature));
        end
        function measure(h, laserData, u, landmark_list)
            observed_LL = landmark_list.getLandmark(laserData, h.x);
            h.observed = observed_LL;
            if ~isempty(observed_LL)
                h.pushParams();
                lm = landmark_list.landmarkObj.landmark;
                ekfslam_mex('measure', h.hnd, double(observed_LL), double(u(:)), double([lm.index]'), ...
                            double(reshape([lm.loc], 2, [])'));
            end
        end
        function removeLandmarks(h, idx)
            % Drop landmarks idx (1-based like every landmark index here; any order, any shape) from the map: their entries of
            % x, their signatures, their rows and columns of P, on the GPU; the survivors keep their order and their bits.
            % Not a method of the reference, which never shrinks its map; WHICH landmark to drop is the caller's policy.
            % Signatures are not renumbered: assign h.s if the UC convention 'new signature = N + 1' would collide.
            h.gateway('remove_landmarks', double(idx(:)));
        end
        function constrainLandmarks(h, i, j, delta, R)
            % 'landmark i minus landmark j was observed as delta (1x2), with noise covariance R (2x2)': a linear EKF correction
            % between two landmarks (1-based, i ~= j), formed and applied on the GPU.  delta = [0 0] says 'the same point';
            % R = zeros(2) is allowed.  Not a method of the reference.
            if nargin < 4 || isempty(delta), delta = [0 0]; end
            if nargin < 5 || isempty(R), R = zeros(2); end
            h.gateway('constrain_landmarks', double(i), double(j), double(delta(:)), double(R));
        end
        function mergeLandmarks(h, keep, drop, R)
            % Fuse two landmarks that are the same point: constrainLandmarks(keep, drop, [0 0], R), then removeLandmarks(drop).
            % keep retains its signature; its number afterwards is keep - (drop < keep).  WHICH pairs to merge is the caller's
            % policy: landmarkDistance is the gate.
            if nargin < 4 || isempty(R), R = zeros(2); end
            h.gateway('merge_landmarks', double(keep), double(drop), double(R));
        end
        function [d2, S] = landmarkDistance(h, i, j, delta, R)
            % Squared Mahalanobis distance of 'landmark i minus landmark j = delta' under the current state, and its 2x2
            % innovation covariance S.  Changes nothing.
            if nargin < 4 || isempty(delta), delta = [0 0]; end
            if nargin < 5 || isempty(R), R = zeros(2); end
            [d2, S] = h.gateway('landmark_distance', double(i), double(j), double(delta(:)), double(R));
        end
        function [d2, partner] = nearestLandmarks(h, R)
            % For every landmark k its closest EARLIER landmark: partner(k) < k minimises landmarkDistance(k, partner(k), [0 0], R)
            % and d2(k) is that minimum; partner(k) = 0 (and d2(k) = Inf) means none -- landmark 1, rows whose pairs are all
            % singular.  The lowest number wins ties.  One read-only pass over P on the GPU; changes nothing.  A row reads as
            % mergeLandmarks(partner(k), k, R); gate d2(k) with a chi-square value (2 degrees of freedom) first.
            if nargin < 2 || isempty(R), R = zeros(2); end
            [d2, partner] = h.gateway('nearest_landmarks', double(R));
        end
        function merges = fuseDuplicates(h, gate, R, maxMerges)
            % The simplest complete fusion policy: search, merge the candidate with the smallest (d2, k) at or below the gate,
            % search again -- until none is left or maxMerges merges were made.  merges: one row [keep drop d2] per fusion.
            if nargin < 3 || isempty(R), R = zeros(2); end
            if nargin < 4 || isempty(maxMerges), maxMerges = Inf; end
            merges = zeros(0, 3);
            while size(merges, 1) < maxMerges
                [d2, partner] = h.nearestLandmarks(R);
                k = find(partner > 0 & d2 <= gate);
                if isempty(k), break; end
                [~, q] = sortrows([d2(k), k]);
                k = k(q(1));
                h.mergeLandmarks(partner(k), k, R);
                merges(end + 1, :) = [partner(k), k, d2(k)]; %#ok<AGROW>
            end
        end
        function d2 = mergeLandmarksBatch(h, pairs, R)
            % Fuse every row [keep drop] of pairs (k x 2, 1-based numbers as they are before the call, k <= 32) in ONE call: what
            % constrainLandmarks(keep, drop, [0 0], R) row by row, then one removeLandmarks(all drops) would leave -- k gathers and
            % one pass over P on the GPU instead of 2 k passes.  A keep may be shared by several rows; no keep may be dropped.
            % d2(r): landmarkDistance(keep_r, drop_r, [0 0], R) as it is just before row r is applied.
            if nargin < 3 || isempty(R), R = zeros(2); end
            d2 = h.gateway('merge_landmarks_batch', double(reshape(pairs, [], 2)), double(R));
        end
        function res = observeLinear(h, z, R, Hr, lm, Hl, gate, wrap, rows, wait)
            % 'H x was observed as z, with noise covariance R' for a constant H: Hr (2x3) on the robot state [x y theta_deg] plus
            % one 2x2 block Hl(:, :, b) on each of the landmarks lm (0, 1 or 2 numbers, 1-based).  An UPDATE-STEP like a correction
            % of measure(): nothing is flushed and, unless wait is true, nothing is waited for.  Applied only if nu' S^-1 nu <= gate;
            % rows named in wrap are angles in degrees (innovation wrapped into (-180, 180]); rows = 1: a scalar observation.
            % wait: res = [nu(1) nu(2) S(:)' d2 outcome] (outcome 1 applied, 2 gated).  Not a method of the reference.
            if nargin < 4 || isempty(Hr), Hr = zeros(2, 3); end
            if nargin < 5, lm = []; end
            if nargin < 6, Hl = []; end
            if nargin < 7 || isempty(gate), gate = Inf; end
            if nargin < 8 || isempty(wrap), wrap = [0 0]; end
            if nargin < 9 || isempty(rows), rows = 2; end
            if nargin < 10 || isempty(wait), wait = false; end
            z = double(z(:)); if numel(z) < 2, z(2) = 0; end
            res = h.gateway('observe_linear', z, double(R), double(Hr), double(lm(:)), double(Hl), double(gate), double(wrap(:)), ...
                            double(rows), double(wait));
        end
        function res = fixLandmark(h, i, pos, R, gate, wait)
            % 'Landmark i is the surveyed point pos, known to within the covariance R': H = eye(2) on that landmark.
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeLinear(pos, R, [], i, eye(2), gate, [0 0], 2, wait);
        end
        function res = fixRobotPosition(h, pos, R, gate, wait)
            % 'The robot is at pos, to within the covariance R' (a GPS fix): Hr = [eye(2) [0; 0]].
            if nargin < 4 || isempty(gate), gate = Inf; end
            if nargin < 5 || isempty(wait), wait = false; end
            res = h.observeLinear(pos, R, [1 0 0; 0 1 0], [], [], gate, [0 0], 2, wait);
        end
        function res = fixRobotHeading(h, thetaDeg, variance, gate, wait)
            % 'The heading reads thetaDeg, with this variance' (a compass): one row, Hr(1, 3) = 1, the innovation wrapped.
            if nargin < 4 || isempty(gate), gate = Inf; end
            if nargin < 5 || isempty(wait), wait = false; end
            res = h.observeLinear([thetaDeg 0], [variance 0; 0 0], [0 0 1; 0 0 0], [], [], gate, [1 0], 1, wait);
        end
        function res = observeModel(h, model, z, R, lm, anchor, gate, wait)
            % 'h(x) was observed as z, with noise covariance R' for a model whose Jacobian depends on the state, linearised on the
            % GPU at the live state: model 1 range and bearing [r; deg], 2 range, 3 bearing (deg, relative to the heading),
            % 4 the target's position in the robot frame [forward; left], 5 the distance between two landmarks.  The target is
            % landmark lm (1-based; two numbers for model 5) or, with lm empty, the known point anchor (1x2) that is not in the
            % map -- then only the robot is corrected.  Bearing innovations are wrapped into (-180, 180].  An UPDATE-STEP like
            % observeLinear: nothing is flushed and, unless wait is true, nothing is waited for; applied only if nu' S^-1 nu <= gate.
            % wait: res = [nu(1) nu(2) S(:)' d2 outcome] (outcome 1 applied, 2 gated).  Not a method of the reference.
            if nargin < 5, lm = []; end
            if nargin < 6, anchor = []; end
            if nargin < 7 || isempty(gate), gate = Inf; end
            if nargin < 8 || isempty(wait), wait = false; end
            z = double(z(:)); if numel(z) < 2, z(2) = 0; end
            if isscalar(R), R = [R 0; 0 0]; end
            res = h.gateway('observe_model', double(model), z, double(R), double(lm(:)), double(anchor(:)), double(gate), double(wait));
        end
        function res = observeModelIterated(h, model, z, R, lm, anchor, gate, iterations, tol, wait)
            % observeModel as the ITERATED EKF update: the model is relinearised on the GPU up to `iterations` times (1..16; default 3)
            % -- Gauss-Newton on the MAP cost over the robot and the target(s) -- until no entry moves by more than tol (default 0: all
            % of them), and the last linearisation makes the step's one pair.  Worth it where the prior is wide against the sensor: a
            % new landmark, a heading known to ten degrees, a precise fix.  One launch, nothing flushed, like observeModel; the gate is
            % read at the first linearisation.  wait: res = [nu(1) nu(2) S(:)' d2 outcome] of the FIRST linearisation (the call's
            % outcome), then [S(:)' nu(1) nu(2) used converged lastStep xLocal(1:7)] of the one that made the pair.  Not a method of
            % the reference.
            if nargin < 5, lm = []; end
            if nargin < 6, anchor = []; end
            if nargin < 7 || isempty(gate), gate = Inf; end
            if nargin < 8 || isempty(iterations), iterations = 3; end
            if nargin < 9 || isempty(tol), tol = 0; end
            if nargin < 10 || isempty(wait), wait = false; end
            z = double(z(:)); if numel(z) < 2, z(2) = 0; end
            if isscalar(R), R = [R 0; 0 0]; end
            res = h.gateway('observe_model_iterated', double(model), z, double(R), double(lm(:)), double(anchor(:)), double(gate), ...
                            double(iterations), double(tol), double(wait));
        end
        function res = observeRangeBearing(h, i, z, R, gate, wait)
            % 'Landmark i is seen at range z(1) and bearing z(2) (degrees, relative to the heading), covariance R'.
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(1, z, R, i, [], gate, wait);
        end
        function res = observeRange(h, i, r, variance, gate, wait)
            % 'Landmark i is at distance r, with this variance' (a range-only beacon).
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(2, [r 0], [variance 0; 0 0], i, [], gate, wait);
        end
        function res = observeBearing(h, i, deg, variance, gate, wait)
            % 'Landmark i is seen at bearing deg (degrees, relative to the heading), with this variance' (a camera).
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(3, [deg 0], [variance 0; 0 0], i, [], gate, wait);
        end
        function res = observeRelativeXY(h, i, z, R, gate, wait)
            % 'Landmark i lies at z = [forward left] in the robot frame, covariance R' (a lidar or stereo front end).
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(4, z, R, i, [], gate, wait);
        end
        function res = observeLandmarkRange(h, i, j, dist, variance, gate, wait)
            % 'Landmarks i and j are dist apart, with this variance' (a tape measure between two beacons).
            if nargin < 6 || isempty(gate), gate = Inf; end
            if nargin < 7 || isempty(wait), wait = false; end
            res = h.observeModel(5, [dist 0], [variance 0; 0 0], [i j], [], gate, wait);
        end
        function res = observeAnchorRange(h, pos, r, variance, gate, wait)
            % 'The known point pos, which is not in the map, is at distance r, with this variance' (a surveyed UWB anchor).
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(2, [r 0], [variance 0; 0 0], [], pos, gate, wait);
        end
        function res = observeAnchorBearing(h, pos, deg, variance, gate, wait)
            % 'The known point pos, which is not in the map, is seen at bearing deg, with this variance'.
            if nargin < 5 || isempty(gate), gate = Inf; end
            if nargin < 6 || isempty(wait), wait = false; end
            res = h.observeModel(3, [deg 0], [variance 0; 0 0], [], pos, gate, wait);
        end
        function idx = addLandmarksModel(h, model, z, R, signature)
            % One scan of NEW landmarks under observeModel's conventions: entry b was seen as z(b, :) through model(b) -- 1 range and
            % bearing [r deg], 4 the position in the robot frame [forward left]; a one-row model does not determine a point -- with
            % noise covariance R(:, :, b) (one 2x2 R: shared by all).  Every entry is inverted on the GPU at the live robot state and
            % the whole scan (at most 32 entries) is appended by one launch; nothing is flushed or waited for.  signature: one per
            % entry; left out or empty, each landmark's own number.  idx: the new landmarks' numbers.  Not a method of the reference,
            % whose append takes the position from the landmark table.
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            if nargin < 5 || isempty(signature), signature = numel(h.s) + (1:m)'; end
            idx = h.gateway('append_model', model, z, R, double(signature(:)));
        end
        function idx = joinMap(h, local, signatureOffset)
            % MAP JOINING: the map of `local` -- another EKF_SLAM / EKF_SLAM_UC object, started at this one's robot pose (x = 0, P = 0 at
            % the moment this one stops moving) and independent of it -- is joined into this one on the GPU: the robot composes with the
            % local robot, the local landmarks follow this map's in the global frame with signature s_local + signatureOffset (left out:
            % 0), and the local map's own cross-covariances are kept.  Both objects are flushed; `local` is otherwise untouched and may
            % be deleted at once.  idx: the new landmarks' numbers.  Follow it with fuseDuplicatesBatched(gate, R) to fuse the landmarks
            % both maps saw.  Not a method of the reference.
            if nargin < 3 || isempty(signatureOffset), signatureOffset = 0; end
            idx = h.gateway('join_map', local.hnd, double(signatureOffset));
        end
        function extractMap(h, idx, frame, dst)
            % MAP EXTRACTION: the robot and landmarks idx (1-based, distinct, any order, any shape) of this map are taken out into `dst`
            % -- another EKF_SLAM / EKF_SLAM_UC object, any tile edge and storage kind, capacity >= numel(idx) -- whose whole state is
            % replaced: its landmark k is landmark idx(k) of this one.  frame 'map' (empty: 'map'): their joint Gaussian as it is, bit
            % for bit; frame 'robot': the landmarks relative to the robot with the robot's own uncertainty folded in, dst's robot at zero
            % with P = 0 -- what joinMap expects of a local map.  On the GPU, O(numel(idx)^2) whatever the size of this map; this object
            % is only flushed.  Follow it with removeLandmarks(idx) to archive a region before dropping it.  Not a method of the reference.
            if isempty(frame), frame = 'map'; end
            switch frame
                case 'map', f = 0;
                case 'robot', f = 1;
                otherwise, error('ekfslam:usage', 'extractMap: frame is ''map'' or ''robot''');
            end
            h.gateway('extract_map', double(idx(:)), f, dst.hnd);
        end
        function transformMap(h, t, Sigma)
            % THE FRAME OF THE MAP: the whole map moved by the rigid transform t = [tx ty phi] (phi in degrees), in place on the GPU: the
            % robot becomes t (+) r, every landmark t(1:2)' + Rot(phi) * l, and P' = T P T' + A Sigma A' with Sigma the 3 x 3 covariance
            % of t itself (left out or empty: an exact transform, the rotation alone) -- georeferencing a finished map into a surveyed
            % frame.  The object keeps its handle and its landmark numbers.  Not a method of the reference.
            if nargin < 3, Sigma = []; end
            h.gateway('transform_map', 0, double(t(:)), double(Sigma));
        end
        function recenterOnRobot(h)
            % The filter re-anchored at the robot: its pose becomes the origin with P(1:3, :) = 0 and every landmark is expressed relative
            % to it, the robot's uncertainty folded into the landmarks -- the robocentric remedy for EKF-SLAM's inconsistency, and the
            % shape joinMap expects of a local map.  Bit for bit extractMap(1:N, 'robot', dst), without a second object.
            h.gateway('transform_map', 1, [], []);
        end
        function [info, d2] = factorMap(h, ref)
            % THE FACTORISATION OF P: one Cholesky factorisation of the covariance on the GPU, of exactly what getP would return, the
            % landmark block eliminated first (rows ascending), the robot last.  info is a struct: n, definite, bad_index (0, or the
            % 1-based index into x of the first pivot that failed in that order), bad_pivot, logdet (NaN where P is not positive
            % definite), logdet_map (the landmark block alone), min_pivot, max_pivot.  ref (left out or empty: none): n x q reference
            % states as columns, q = 1 .. 8; d2(k) = (x - ref(:,k))' * inv(P) * (x - ref(:,k)) with the heading difference wrapped --
            % the NEES against ground truth.  Read-only.  Not a method of the reference.
            if nargin < 2, ref = []; end
            [v, d2] = h.gateway('factor_map', double(ref));
            info = struct('n', v(1), 'definite', v(2) ~= 0, 'bad_index', v(3), 'bad_pivot', v(4), 'logdet', v(5), 'logdet_map', v(6), ...
                          'min_pivot', v(7), 'max_pivot', v(8));
        end
        function [samples, info] = sampleMap(h, xi)
            % DRAWS FROM THE POSTERIOR: samples(:, q) = x + C * xi(:, q) for the k columns of xi (n x k, n = 3 + 2 N; randn(n, k) for
            % samples of the Gaussian the filter carries), from ONE factorisation on the GPU.  C is the lower-triangular Cholesky factor
            % of P in factorMap's elimination order (the landmark block first, the robot last) mapped back to x's order: C * C' = P.
            % The heading entry is not wrapped.  info is factorMap's struct; where P is not positive definite samples is all NaN.
            % Read-only.  Not a method of the reference.
            [samples, v] = h.gateway('sample_map', double(xi));
            info = struct('n', v(1), 'definite', v(2) ~= 0, 'bad_index', v(3), 'bad_pivot', v(4), 'logdet', v(5), 'logdet_map', v(6), ...
                          'min_pivot', v(7), 'max_pivot', v(8));
        end
        function [out, info] = solveMap(h, B, form)
            % THE OTHER DIRECTION: out(:, q) = P \ B(:, q) (form 'full', the default) or the whitened C \ B(:, q) in x's order
            % (form 'half': sum(out(:, q).^2) = B(:, q)' * (P \ B(:, q))) for the k columns of B (n x k, n = 3 + 2 N), from ONE
            % factorisation on the GPU.  C is the Cholesky factor of P in factorMap's elimination order (the landmark block first, the
            % robot last).  No entry is wrapped.  info is factorMap's struct; where P is not positive definite out is all NaN.
            % Read-only.  Not a method of the reference.
            if nargin < 3, form = 'full'; end
            [out, v] = h.gateway('solve_map', double(B), double(strcmp(form, 'half')));
            info = struct('n', v(1), 'definite', v(2) ~= 0, 'bad_index', v(3), 'bad_pivot', v(4), 'logdet', v(5), 'logdet_map', v(6), ...
                          'min_pivot', v(7), 'max_pivot', v(8));
        end
        function out = multiplyMap(h, B)
            % THE PLAIN PRODUCT: out(:, q) = P * B(:, q) for the k columns of B (n x k, n = 3 + 2 N), P exactly what getP reports, with
            % NO factorisation: one read-only pass over the tiled P on the GPU per 16 columns.  A * multiplyMap(A') is the covariance
            % of the linear functions A * x; unit vectors return columns of P; P * z - b checks a solveMap answer.  No entry is
            % wrapped.  Read-only.  Not a method of the reference.
            out = h.gateway('multiply_map', double(B));
        end
        function [res, nu, S] = observeDense(h, H, z, R, gate, wrap)
            % A LINEAR OBSERVATION WITH A DENSE H: 'H * x = z +- R' for k <= 16 rows (H: k x n, n = 3 + 2 N) that may touch EVERY landmark
            % -- the fix of a group's centroid, displacement constraints applied jointly, conditioning with R = 0.  Exact, applied only
            % if d2 <= gate (default Inf); wrap: the rows whose innovation is an angle in degrees (default none).  One product pass and
            % one update pass over the tiled P on the GPU.  res: struct with d2, rows, outcome (1 applied, 2 gated) and bad_row; an S
            % that is not positive definite is an error and changes nothing.  Not a method of the reference.
            if nargin < 5, gate = Inf; end
            if nargin < 6, wrap = []; end
            [v, nu, S] = h.gateway('observe_dense', double(H).', double(z), double(R), double(gate), double(wrap));
            res = struct('d2', v(1), 'rows', v(2), 'outcome', v(3), 'bad_row', v(4));
        end
        function idx = addLandmarkRangeBearing(h, z, R, signature)
            % 'A landmark that is not in the map yet is seen at range z(1) and bearing z(2) (degrees, relative to the heading),
            % covariance R': it joins the map at the point that observation names.
            if nargin < 4, signature = []; end
            idx = h.addLandmarksModel(1, z(:)', R, signature);
        end
        function idx = addLandmarkRelativeXY(h, z, R, signature)
            % 'A landmark that is not in the map yet lies at z = [forward left] in the robot frame, covariance R'.
            if nargin < 4, signature = []; end
            idx = h.addLandmarksModel(4, z(:)', R, signature);
        end
        function predictModel(h, model, u, M)
            % MOTION under observeModel's conventions: step b moves the robot by u(b, :) through model(b) -- 1 turn-then-drive
            % [d deg], 2 an arc [length deg], 3 a pose increment in the robot frame [dx dy deg] -- and u has the covariance
            % M(:, :, b) (2x2 for models 1 and 2, 3x3 for model 3, or 3x3 throughout with the leading block in use; one M: shared by
            % all).  x_r <- f(x_r, u), P <- F P F' + V M V' with the true Jacobians (theta in degrees: the factor pi/180 where it
            % belongs), the whole chain (at most 32 steps) in order by one launch; nothing is flushed or waited for.  Not a method of
            % the reference, whose predict keeps F at the pre-motion heading without pi/180 and a rank-one Q.
            model = double(model(:)); m = numel(model);
            u = double(u); if size(u, 1) ~= m, u = reshape(u, m, []); end
            u(:, end + 1:3) = 0;
            M = double(M); if size(M, 3) == 1, M = repmat(M, [1 1 m]); end
            M3 = zeros(3, 3, m); M3(1:size(M, 1), 1:size(M, 2), :) = M;
            h.gateway('predict_model', model, u, M3);
        end
        function predictTurnDrive(h, d, deg, M)
            % 'The robot turned by deg degrees, then drove d; [d deg] has the covariance M (2x2)'; vectors d, deg: a chain of steps.
            h.predictModel(ones(numel(d), 1), [d(:) deg(:)], M);
        end
        function predictArc(h, d, deg, M)
            % 'The robot drove an arc of length d while turning by deg degrees; [d deg] has the covariance M (2x2)'.
            h.predictModel(2 * ones(numel(d), 1), [d(:) deg(:)], M);
        end
        function predictPoseDelta(h, dx, dy, deg, M)
            % 'The pose changed by [dx dy deg] in the robot frame, with covariance M (3x3)'; zeros: additive noise M in the robot frame.
            h.predictModel(3 * ones(numel(dx), 1), [dx(:) dy(:) deg(:)], M);
        end
        function [match, d2] = associateModel(h, model, z, R, gate)
            % WHICH landmark each sighting of a scan belongs to, under observeModel's conventions: observation k was seen as z(k, :)
            % through model(k) (1 range and bearing, 2 range, 3 bearing, 4 the position in the robot frame) with noise covariance
            % R(:, :, k) (one 2x2 R: shared by all).  match: one row [best second d2best d2second withinGate irregular] per
            % observation -- the landmarks with the smallest and second-smallest d2 (0 = none, d2 = Inf), how many landmarks have
            % d2 <= gate(k) (one gate: shared; default Inf), how many have no d2.  Every d2 is what observeModel would report for
            % that pair.  d2 (optional): N x m, column k = observation k against every landmark (NaN where a pair has no d2).  One
            % small launch for the whole scan; changes and flushes nothing.  Not a method of the reference.
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            if nargin < 5 || isempty(gate), gate = Inf; end
            gate = double(gate(:)); if isscalar(gate), gate = repmat(gate, m, 1); end
            if nargout > 1
                [match, d2] = h.gateway('associate_model', model, z, R, gate);
            else
                match = h.gateway('associate_model', model, z, R, gate);
            end
        end
        function [res, total, cand, candD2] = assignModel(h, model, z, R, gate)
            % WHICH observation of a scan gets WHICH landmark when they compete: the one-to-one assignment that minimises the summed
            % d2, with gate(k) (one gate: shared; finite) as the price of leaving observation k out; arguments as for associateModel.
            % res: one row [landmark d2 ncand best second d2best d2second withinGate irregular] per observation -- the landmark it is
            % assigned to (0 = left out, d2 = Inf), how many candidates (landmarks with d2 <= gate, at most 32) were kept, and
            % associateModel's record.  total: the minimised sum.  cand, candD2 (optional): m x 32, row k = the kept candidates of
            % observation k by (d2, landmark), 0 / Inf behind them.  Decided on the device; changes and flushes nothing.  Not a
            % method of the reference.
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            gate = double(gate(:)); if isscalar(gate), gate = repmat(gate, m, 1); end
            if nargout > 2
                [res, total, cand, candD2] = h.gateway('assign_model', model, z, R, gate);
            else
                [res, total] = h.gateway('assign_model', model, z, R, gate);
            end
        end
        function out = measureModelAssigned(h, model, z, R, gateMatch, gateNew, signature)
            % measureModel with the ambiguity discard replaced by the global-nearest-neighbour ASSIGNMENT: ONE assignModel call with
            % gate = gateMatch, then: an observation is MATCHED when it has an assigned landmark, NEW when no landmark lies inside
            % gateMatch (ncand == 0) and d2best > gateNew or the map is empty (gateNew >= gateMatch), DISCARDED otherwise.  The
            % matched ones go to observeModel(..., landmark, [], gateMatch) in scan order, then ALL new ones to one
            % addLandmarksModel call.  out: one row [kind landmark] per observation, kind 1 matched, 2 new, 0 discarded
            % (landmark 0).  Not a method of the reference.
            if ~(gateNew >= gateMatch), error('EKF_SLAM:measureModelAssigned', 'gateNew >= gateMatch is required'); end
            model = double(model(:)); m = numel(model);
            if any(model ~= 1 & model ~= 4), error('EKF_SLAM:measureModelAssigned', 'model is 1 or 4: a one-row model does not start a landmark'); end
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            if nargin < 7, signature = []; end
            res = h.assignModel(model, z, R, gateMatch);
            kind = zeros(m, 1);
            kind(res(:, 1) > 0) = 1;
            kind(kind == 0 & res(:, 3) == 0 & (res(:, 4) == 0 | res(:, 6) > gateNew)) = 2;
            out = zeros(m, 2);
            for k = find(kind == 1)'
                h.observeModel(model(k), z(k, :), R(:, :, k), res(k, 1), [], gateMatch, false);
                out(k, :) = [1 res(k, 1)];
            end
            fresh = find(kind == 2);
            if ~isempty(fresh)
                if isempty(signature), sig = []; else, sig = signature(fresh); end
                out(fresh, 1) = 2;
                out(fresh, 2) = h.addLandmarksModel(model(fresh), z(fresh, :), R(:, :, fresh), sig);
            end
        end
        function out = measureModel(h, model, z, R, gateMatch, gateNew, signature)
            % One scan under observeModel's conventions, observe-or-append (models 1 and 4): ONE associateModel call with
            % gate = gateMatch, then: an observation is MATCHED when exactly one landmark lies inside gateMatch (that landmark, its
            % best), NEW when d2best > gateNew or the map is empty (gateNew >= gateMatch), DISCARDED otherwise (ambiguous, or
            % between the gates).  Where several are matched to one landmark the smallest d2best keeps it (the lower row on a tie),
            % the others are discarded.  The matched ones go to observeModel(..., landmark, [], gateMatch) in scan order, then ALL
            % new ones to one addLandmarksModel call.  out: one row [kind landmark] per observation, kind 1 matched, 2 new,
            % 0 discarded (landmark 0).  Not a method of the reference.
            if ~(gateNew >= gateMatch), error('EKF_SLAM:measureModel', 'gateNew >= gateMatch is required'); end
            model = double(model(:)); m = numel(model);
            if any(model ~= 1 & model ~= 4), error('EKF_SLAM:measureModel', 'model is 1 or 4: a one-row model does not start a landmark'); end
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            if nargin < 7, signature = []; end
            match = h.associateModel(model, z, R, gateMatch);
            kind = zeros(m, 1);
            kind(match(:, 5) == 1) = 1;
            kind(kind == 0 & (match(:, 1) == 0 | match(:, 3) > gateNew)) = 2;
            for k = find(kind == 1)'
                rivals = find(kind == 1 & match(:, 1) == match(k, 1));
                [~, w] = min(match(rivals, 3));                  % the first minimum: the lower row on a tie
                if rivals(w) ~= k, kind(k) = -1; end
            end
            kind(kind == -1) = 0;
            out = zeros(m, 2);
            for k = find(kind == 1)'
                h.observeModel(model(k), z(k, :), R(:, :, k), match(k, 1), [], gateMatch, false);
                out(k, :) = [1 match(k, 1)];
            end
            fresh = find(kind == 2);
            if ~isempty(fresh)
                if isempty(signature), sig = []; else, sig = signature(fresh); end
                out(fresh, 1) = 2;
                out(fresh, 2) = h.addLandmarksModel(model(fresh), z(fresh, :), R(:, :, fresh), sig);
            end
        end
        function [res, prefix] = jointInnovation(h, model, z, R, hyp)
            % The JOINT compatibility of a scan's pairings, under observeModel's conventions: hyp(i, k) is the landmark observation k
            % (model(k), z(k, :), R(:, :, k) as for associateModel) is paired with in hypothesis i, 0 = left out.  res: one row
            % [d2 dof pairings outcome firstIrregular] per hypothesis -- d2 = nu' * inv(S) * nu over the stacked paired rows with
            % S = H*P*H' + blkdiag(R), what a joint-compatibility search tests against the chi-square quantile of dof; outcome 1 regular,
            % 0 irregular (d2 NaN; firstIrregular: the entry of the scan, 0 = none).  prefix (optional): nh x m, the joint d2 of the
            % pairings among observations 1..k.  At most 256 hypotheses a call; changes and flushes nothing.  Not a method of the reference.
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            hyp = double(reshape(hyp, [], m));
            if nargout > 1
                [res, prefix] = h.gateway('joint_innovation', model, z, R, hyp);
            else
                res = h.gateway('joint_innovation', model, z, R, hyp);
            end
        end
        function [res, lm, match] = jointSearch(h, model, z, R, gate, threshold, beam)
            % The joint-compatibility SEARCH over a scan on the device, one wait: entries as for jointInnovation, gate the candidate gate of
            % every entry (finite), threshold(dof + 1) the bound of a joint d2 with dof real rows (dof = 0 .. 2m, e.g. chi-square quantiles),
            % beam at most 64 (default 64).  Level k extends every alive hypothesis by the 4 closest candidates of entry k and by "left out".
            % res = [d2 dof pairings truncated nalive irregular] of the winner; lm(k): the landmark entry k is paired with, 0 = left out;
            % match: one row [withinGate best d2Best] per entry (withinGate == 0: no candidate).  Changes and flushes nothing.  Not a method
            % of the reference.
            if nargin < 7, beam = 64; end
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            [res, lm, match] = h.gateway('joint_search', model, z, R, double(gate), double(threshold(:)), double(beam));
        end
        function res = observeModelJoint(h, model, z, R, lm, gate)
            % One hypothesis of jointInnovation APPLIED as one joint update: lm(k) is the landmark observation k (model(k), z(k, :),
            % R(:, :, k)) is paired with, 0 = left out.  All pairings are linearised once, at the live state, and stacked -- the update
            % whose joint d2 is reported, independent of scan order, one pass over P -- and applied only if d2 <= gate (default Inf).
            % res = [d2 dof pairings outcome firstIrregular], outcome 1 applied, 2 gated; a pairing without a d2 is an error and changes
            % nothing.  The pending corrections are applied first.  Not a method of the reference.
            if nargin < 6 || isempty(gate), gate = Inf; end
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            res = h.gateway('observe_model_joint', model, z, R, double(lm(:)), double(gate));
        end
        function res = observeModelJointIterated(h, model, z, R, lm, gate, iterations, tol)
            % observeModelJoint RELINEARISED: Gauss-Newton over the robot and the paired landmarks, up to `iterations` linearisations
            % (1..16, default 3), stopping where no entry moves by more than tol (default 0); the last linearisation is applied.  The gate
            % is read at the first one.  res = [d2 dof pairings outcome firstIrregular used converged step], the first five the first
            % linearisation's; an iterate that is irregular is an error and changes nothing.  Not a method of the reference.
            if nargin < 6 || isempty(gate), gate = Inf; end
            if nargin < 7 || isempty(iterations), iterations = 3; end
            if nargin < 8 || isempty(tol), tol = 0; end
            model = double(model(:)); m = numel(model);
            z = double(reshape(z, [], 2));
            R = double(R); if size(R, 3) == 1, R = repmat(R, [1 1 m]); end
            res = h.gateway('observe_model_joint_iterated', model, z, R, double(lm(:)), double(gate), double(iterations), double(tol));
        end
        function merges = fuseDuplicatesBatched(h, gate, R, maxMerges)
            % fuseDuplicates with the pairs of one search fused in one mergeLandmarksBatch call: search; walk the candidates in
            % (d2, k) order and take [partner(k) k] when k is not yet a keep or a drop and partner(k) is not yet a drop (a keep may
            % be shared); one batch; search again -- until no candidate is left or maxMerges merges were made.
            % merges: one row [keep drop d2] per fusion, d2 as the batch call reported it.
            if nargin < 3 || isempty(R), R = zeros(2); end
            if nargin < 4 || isempty(maxMerges), maxMerges = Inf; end
            merges = zeros(0, 3);
            while size(merges, 1) < maxMerges
                [d2, partner] = h.nearestLandmarks(R);
                k = find(partner > 0 & d2 <= gate);
                if isempty(k), break; end
                [~, q] = sortrows([d2(k), k]);
                k = k(q);
                limit = min(32, maxMerges - size(merges, 1));
                pairs = zeros(0, 2);
                for r = 1:numel(k)
                    if size(pairs, 1) >= limit, break; end
                    i = k(r); j = partner(i);
                    if any(pairs(:) == i) || any(pairs(:, 2) == j), continue; end
                    pairs(end + 1, :) = [j, i]; %#ok<AGROW>
                end
                dd = h.mergeLandmarksBatch(pairs, R);
                merges = [merges; pairs, dd(:)]; %#ok<AGROW>
            end
        end
        function B = covarianceBlock(h, r0, c0, nr, nc)   % P(r0:r0+nr-1, c0:c0+nc-1) without moving the rest of P
            B = ekfslam_mex('get_P_block', h.hnd, r0, c0, nr, nc);
        end
        function plot(h, landmark_list)
            % Same figure content as the reference's plot (robot, landmarks, the landmark source's own overlay, one
            % covariance ellipse per 2x2 diagonal block) from TWO device reads: x and the diagonal blocks
            % (the reference indexes the full h.P, EKF_SLAM.m:180,205 -- 3.2 GB at 10k landmarks).
            xs = h.x;
            B = reshape(ekfslam_mex('get_P_diag_blocks', h.hnd), 2, 2, []);
            hold on;
            if exist('drawRobot', 'file'), drawRobot(xs(1), xs(2), xs(3), 0.25); end
            if numel(xs) > 3, scatter(xs(4:2:end), xs(5:2:end), 'blue', 'x'); end
            if nargin > 1 && ~isempty(landmark_list)
                landmark_list.landmarkObj.plot(xs, h.observed);
            end
            EKF_SLAM.ellipse(B(:, :, 1), xs(1:2), 0.25);
            for k = 2:size(B, 3)
                EKF_SLAM.ellipse(B(:, :, k), xs(2 * k:2 * k + 1), 0.50);
            end
            hold off;
        end
    end
    methods (Static)
        function ellipse(Sigma, mu, shrink)
            % boundary of { mu + shrink * 2 * sqrt(chi2) * Sigma^(1/2) * [cos t; sin t] }
            if any(isnan(Sigma(:))), return; end            % block held by another shard
            [V, D] = eig((Sigma + Sigma') / 2);
            t = linspace(-pi, pi, 629);
            pts = V * (2 * sqrt(2.2788 * max(D, 0))) * [cos(t); sin(t)] * shrink;
            plot(pts(1, :) + mu(1), pts(2, :) + mu(2));
        end
    end
    methods (Access = protected)
        function m = abiMode(~), m = 0; end               % EKF_MODE_KNOWN
        function varargout = gateway(h, cmd, varargin)    % ekfslam_mex(cmd, handle, args...) for commands added after the core set
            [varargout{1:nargout}] = ekfslam_mex(cmd, h.hnd, varargin{:});
        end
    end
end
