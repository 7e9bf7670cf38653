!  qn_idx_dev -- qn_shift_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's
!  built-in separable bounded quadratic, classic entry setulb_dev) to a NEW_X return, then the marginal covariance of
!  three parameters -- the first free row, the first free row from n / 2 on and the last free row (lbfgsb_kkt's status) --
!  without a vector of length n: the 3 x 3 block of H = B^-1 at those indices (lbfgsb_qn_block) and its correlations,
!  and the same from the model pinned at the active rows, (B + D)^-1 with d_i = +inf on the rows at a bound
!  (lbfgsb_qn_shift_set, lbfgsb_qn_shift_block).  Then the stored pairs' rows there (lbfgsb_qn_rows) and the columns at
!  the three indices (lbfgsb_qn_cols, lbfgsb_qn_shift_cols), whose entries at the indices must be the blocks'.
!
!     qn_idx_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNIDX col = <stored pairs> pinned = <pinned rows>
!     QNIDX idx <the three global 0-based indices>
!     QNIDX H <row> <three entries>            the marginal covariance under N(x, H), three rows
!     QNIDX Hcorr <row> <three entries>        its correlations
!     QNIDX S <row> <three entries>            the same with the active rows held fixed
!     QNIDX Scorr <row> <three entries>
!     QNIDX rows <largest |entry| of the gathered rows of [S, Y]>
!     QNIDX cols <largest |column entry - block entry| for H> <the same for the pinned model>
      program qn_idx_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit
      use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_positive_inf

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: ah(3, 3), as(3, 3), rows(3, 2048), rmax, ch, cs
      integer(c_int64_t)    :: idx(3), none(1)
      integer               :: j, col
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, du1, dhu, dd, dstatus
      real(wp), allocatable, target :: hu(:), hd(:)
      integer(c_int8_t), allocatable, target :: hstatus(:)
      integer(c_int64_t)    :: cnt(LBFGSB_KKT_NCNT), pinned
      real(c_double)        :: val(LBFGSB_KKT_NVAL)
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(du1, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dhu, vbytes), 'hipMalloc H u')
      call chk(hipMalloc(dd, vbytes), 'hipMalloc d')
      call chk(hipMalloc(dstatus, int(n, c_size_t)), 'hipMalloc status')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the rows at a bound at this iterate (codes 1, 2, 3 of lbfgsb_kkt's status) are pinned, the others not shifted
      call lbfgsb_kkt(ctx, dx, dl, du, dnbd, dg, 0.0_c_double, c_null_ptr, c_null_ptr, dstatus, cnt, val, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      allocate (hstatus(n), hd(n), hu(n))
      call chk(hipMemcpy(c_loc(hstatus), dstatus, int(n, c_size_t), D2H), 'hipMemcpy status')
      do i = 1, n
         if (hstatus(i) >= 1_c_int8_t) then
            hd(i) = ieee_value(1.0_wp, ieee_positive_inf)
         else
            hd(i) = 0.0_wp
         end if
      end do
      call chk(hipMemcpy(dd, c_loc(hd), vbytes, H2D), 'hipMemcpy d')
      call lbfgsb_qn_shift_set(ctx, dd, 0.0_c_double, pinned, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_set failed: ', lbfgsb_error_message()
         error stop 1
      end if
      col = isave(28)
      write (output_unit, '(a,i4,a,i0)') 'QNIDX col =', col, ' pinned = ', pinned
      ! three free rows, as global 0-based indices
      idx = -1_c_int64_t
      do i = 1, n
         if (hstatus(i) < 1_c_int8_t) then
            if (idx(1) < 0) idx(1) = int(i - 1, c_int64_t)
            if (idx(2) < 0 .and. i - 1 >= n/2) idx(2) = int(i - 1, c_int64_t)
            idx(3) = int(i - 1, c_int64_t)
         end if
      end do
      if (idx(1) < 0 .or. idx(2) < 0) error stop 4
      write (output_unit, '(a,3(1x,i0))') 'QNIDX idx', idx
      none = 0_c_int64_t
      call lbfgsb_qn_block(ctx, LBFGSB_QN_H, 3, idx, 0, none, ah, 3, rc)
      if (rc == 0) call lbfgsb_qn_shift_block(ctx, 3, idx, 0, none, as, 3, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_block / lbfgsb_qn_shift_block failed: ', lbfgsb_error_message()
         error stop 1
      end if
      do i = 1, 3
         write (output_unit, '(a,i2,3es25.16e3)') 'QNIDX H', i, (ah(i, j), j = 1, 3)
      end do
      do i = 1, 3
         write (output_unit, '(a,i2,3es25.16e3)') 'QNIDX Hcorr', i, (ah(i, j)/sqrt(ah(i, i)*ah(j, j)), j = 1, 3)
      end do
      do i = 1, 3
         write (output_unit, '(a,i2,3es25.16e3)') 'QNIDX S', i, (as(i, j), j = 1, 3)
      end do
      do i = 1, 3
         write (output_unit, '(a,i2,3es25.16e3)') 'QNIDX Scorr', i, (as(i, j)/sqrt(as(i, i)*as(j, j)), j = 1, 3)
      end do
      ! the rows of the stored pairs at the indices, and the columns there against the blocks
      rows = 0.0_c_double
      call lbfgsb_qn_rows(ctx, 3, idx, rows, 3, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_rows failed: ', lbfgsb_error_message()
         error stop 1
      end if
      rmax = 0.0_c_double
      do j = 1, min(2*col, 2048)
         do i = 1, 3
            rmax = max(rmax, abs(rows(i, j)))
         end do
      end do
      write (output_unit, '(a,es25.16e3)') 'QNIDX rows', rmax
      ch = 0.0_c_double; cs = 0.0_c_double
      do j = 1, 3
         call lbfgsb_qn_cols(ctx, LBFGSB_QN_H, 1, idx(j:j), du1, n, rc)
         if (rc == 0) call lbfgsb_qn_shift_cols(ctx, 1, idx(j:j), dhu, n, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' lbfgsb_qn_cols / lbfgsb_qn_shift_cols failed: ', lbfgsb_error_message()
            error stop 1
         end if
         call chk(hipMemcpy(c_loc(hu), du1, vbytes, D2H), 'hipMemcpy column of H')
         call chk(hipMemcpy(c_loc(hbuf), dhu, vbytes, D2H), 'hipMemcpy column of the pinned model')
         do i = 1, 3
            ch = max(ch, abs(real(hu(idx(i) + 1), c_double) - ah(i, j)))
            cs = max(cs, abs(real(hbuf(idx(i) + 1), c_double) - as(i, j)))
         end do
      end do
      write (output_unit, '(a,2es25.16e3)') 'QNIDX cols', ch, cs
      deallocate (hstatus, hd, hu)

      task = 'STOP: QN_IDX_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(du1); rc = hipFree(dnbd); rc = hipFree(dhu); rc = hipFree(dd); rc = hipFree(dstatus)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_idx_dev
